"""CPU tests of the depth noise (giga_depth_noise, giga_amd.noise): the numpy restatement (tests/noise_emu.py) against the
reference's own vgn.utils.misc functions run on the same draws (tests/golden/g18_depth_noise.npz, tools/make_noise_goldens.py),
the distribution and independence of the draw streams, the C ABI's argument checks (made before the first HIP call, so they run
without a GPU) and the argument handling of the Python surface."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch
from scipy import stats

import noise_emu as N
import tsdf_emu as emu
from giga_amd import _capi, noise, perception

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_depth_noise.npz")
F32 = np.float32


@pytest.fixture(scope="module")
def g18():
    return np.load(GOLDEN)


def within_one_ulp(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / N.ulp32(want)
    print(f"{what}: max {err.max():.3g} ulp, {int((err > 0).sum())} of {err.size} differ")
    assert err.max() <= 1.0, what


@pytest.mark.parametrize("shape", N.SMALL_SHAPES + [N.BIG_SHAPE], ids=lambda s: "%dx%d" % s)
def test_emulation_equals_the_reference_functions(g18, shape):
    H, W = shape
    tag = "%dx%d" % shape
    ids, seed = N.IDS[shape], int(g18["seed"])
    assert seed == N.FIXTURE_SEED and [int(i) for i in g18["ids_" + tag]] == ids
    imgs = N.depth_images(len(ids), H, W, int(g18["image_seed"]))
    assert np.array_equal(np.frombuffer(hashlib.sha256(imgs.tobytes()).digest(), np.uint8), g18["in_sha_" + tag])
    on = g18["dex_on_" + tag]
    assert on.any() and not on.all()
    assert np.array_equal(on, N.coin(np.array(ids, np.uint64), seed) < 0.5)
    big = shape == N.BIG_SHAPE
    sub = (slice(None), slice(None, None, N.BIG_STRIDE[0]), slice(None, None, N.BIG_STRIDE[1])) if big else (slice(None),) * 3
    for kind in ("dex", "trans", "norm"):
        out = N.apply(kind, imgs, ids, seed)
        within_one_ulp(out[sub], g18[kind + "_" + tag], f"{kind} {tag}")
        if big:
            sums = out.astype(np.float64).sum(axis=(1, 2))
            # every pixel within one float32 ulp (< 2^-22 of values below 4): the sums agree to that, times the pixel count
            assert np.all(np.abs(sums - g18[kind + "_sum_" + tag]) <= H * W * 2.0 ** -22), (kind, sums, g18[kind + "_sum_" + tag])
    for i, image_id in enumerate(ids):
        _, _, r, c = N.trans_coords(H, W, image_id, seed)
        assert np.array_equal(r[sub[1:]], g18["r_" + tag][i]) and np.array_equal(c[sub[1:]], g18["c_" + tag][i])
        # the test images make a wrong gather visible: neighbouring sources differ
        assert len(np.unique(imgs[i])) > H * W // 4


def test_upsample_is_the_unclipped_resize():
    """noise_emu.upsample against scipy.ndimage.zoom(order=1, mode='grid-constant', grid_mode=True): what
    skimage.transform.resize(order=1, mode='constant', anti_aliasing=False) evaluates before its clip"""
    import scipy.ndimage
    rng = np.random.default_rng(0)
    for (H, W), (h, w) in (((24, 36), (6, 9)), ((30, 45), (7, 11)), ((9, 5), (2, 1)), ((4, 4), (1, 1)), ((65, 130), (21, 43))):
        g = rng.standard_normal((h, w))
        want = scipy.ndimage.zoom(g, (H / h, W / w), order=1, mode="grid-constant", cval=0.0, grid_mode=True)
        assert want.shape == (H, W) and np.abs(N.upsample(g, H, W) - want).max() < 1e-15


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_draw_distributions(seed):
    n = 20000
    p_normal = stats.kstest(N.normals(n, 0, N.STREAM_PIXEL, seed), "norm").pvalue
    p_uniform = stats.kstest(N.coin(np.arange(n), seed), "uniform").pvalue
    g, used = N.gamma(np.arange(n), seed)
    p_gamma = stats.kstest(g, "gamma", args=(1000, 0, 0.001)).pvalue
    print(f"seed {seed}: p normal {p_normal:.3g}, uniform {p_uniform:.3g}, gamma {p_gamma:.3g}; most gamma attempts {used.max()}")
    assert min(p_normal, p_uniform, p_gamma) > 1e-4
    assert used.max() < N.GAMMA_ATTEMPTS
    u = np.concatenate(N.uniform_pairs(np.arange(n), 0, N.STREAM_GP, seed))
    assert u.min() > 0.0 and u.max() < 1.0


def test_uniform_is_strictly_inside_the_unit_interval():
    lo, hi = np.zeros(1, np.uint32), np.full(1, 0xffffffff, np.uint32)
    assert N.u53(lo, lo)[0] == 2.0 ** -54 and N.u53(hi, hi)[0] == 1.0 - 2.0 ** -53
    assert N.u53(lo, np.full(1, 64, np.uint32))[0] == 2.0 ** -53


def test_gamma_cap_falls_back_to_the_documented_value():
    """with no attempt allowed the draw is (shape - 1/3) scale, the sampler's value at x = 0"""
    g, used = N.gamma(np.arange(4), 0, attempts=0)
    assert np.all(g == (1000.0 - 1.0 / 3.0) * 0.001) and np.all(used == 0)


def test_streams_and_images_are_independent():
    n = 20000
    bound = 4.0 / np.sqrt(n)
    z = {(s, i): N.normals(n, i, s, 0) for s in (N.STREAM_GP, N.STREAM_ROW, N.STREAM_COL, N.STREAM_PIXEL) for i in (0, 1)}
    keys = sorted(z)
    for a in range(len(keys)):
        for b in range(a + 1, len(keys)):
            r = np.corrcoef(z[keys[a]], z[keys[b]])[0, 1]
            assert abs(r) < bound, (keys[a], keys[b], r)
    other = N.normals(n, 1 << 32, N.STREAM_PIXEL, 0)              # the high word of the id is part of the counter
    assert abs(np.corrcoef(other, z[(N.STREAM_PIXEL, 0)])[0, 1]) < bound and not np.array_equal(other, z[(N.STREAM_PIXEL, 0)])
    assert abs(np.corrcoef(N.normals(n, 0, N.STREAM_PIXEL, 1), z[(N.STREAM_PIXEL, 0)])[0, 1]) < bound
    # the two normals of a block, and neighbouring elements
    assert abs(np.corrcoef(z[(N.STREAM_PIXEL, 0)][0::2], z[(N.STREAM_PIXEL, 0)][1::2])[0, 1]) < 4.0 / np.sqrt(n // 2)
    g0, g1 = N.gamma(np.arange(n), 0)[0], N.gamma(np.arange(n), 1)[0]
    assert abs(np.corrcoef(g0, g1)[0, 1]) < bound and abs(np.corrcoef(g0, N.coin(np.arange(n), 0))[0, 1]) < bound


# ------------------------------------------------------------------------------------------------------------------ C ABI
IN, OUT, WS = 0x10000000, 0x20000000, 0x30000000          # never dereferenced: every check precedes the first HIP call


def call(n=2, W=8, H=8, model=1, params=None, src=IN, dst=OUT, ws=WS, ws_bytes=1 << 20, ids=None):
    L = _capi.lib()
    p = np.asarray(params, np.float64) if params is not None else None
    i = np.asarray(ids, np.uint64) if ids is not None else None
    return L.giga_depth_noise(src, dst, n, W, H, model, p.ctypes.data if p is not None else None, 7,
                              i.ctypes.data if i is not None else None, ws, ws_bytes, None)


def test_abi_argument_checks_without_a_gpu():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_depth_noise", "giga_depth_noise_workspace_bytes"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    assert "#define GIGA_NOISE_GAMMA_ATTEMPTS %d\n" % N.GAMMA_ATTEMPTS in hdr
    for k, v in _capi.NOISE_MODEL.items():
        assert "#define GIGA_NOISE_%s %d\n" % (k.upper(), v) in hdr
    big = 16384                                            # GIGA_TSDF_MAX_IMAGE
    assert "#define GIGA_TSDF_MAX_IMAGE %d\n" % big in hdr
    for model in (1, 2, 3):
        assert call(n=0, model=model, src=None, dst=None, ws=None, ws_bytes=0) == 0
        assert call(n=-1, model=model) == -1
        for W, H in ((0, 8), (8, 0), (big + 1, 8), (8, big + 1)):
            assert call(W=W, H=H, model=model) == -1
        assert call(n=8, W=big, H=big, model=model) == -1                       # n W H = 2^31
        assert call(model=model, src=None) == -1 and call(model=model, dst=None) == -1 and call(model=model, ws=None) == -1
        need = L.giga_depth_noise_workspace_bytes(2, 8, 8, model)
        assert need >= 16 and call(model=model, ws_bytes=need - 1) == -4
        # aliasing: equal, overlapping from either side; touching ranges are fine for the check (they fail only at the size test)
        bytes_ = 2 * 8 * 8 * 4
        assert call(model=model, dst=IN) == -1 and call(model=model, dst=IN + bytes_ - 4) == -1 and call(model=model, dst=IN - bytes_ + 4) == -1
        assert call(model=model, dst=IN + bytes_, ws_bytes=0) == -4 and call(model=model, dst=IN - bytes_, ws_bytes=0) == -4
    assert call(model=0) == -1 and call(model=4) == -1
    assert L.giga_depth_noise_workspace_bytes(2, 8, 8, 0) == 0 and L.giga_depth_noise_workspace_bytes(0, 8, 8, 1) == 0
    dex = [1000.0, 0.001, 0.005, 4.0, 0.5]
    assert call(params=dex, ws_bytes=0) == -4                                    # valid: reaches the size test
    for i in range(4):
        for bad in (0.0, -1.0, np.nan, np.inf):
            assert call(params=dex[:i] + [bad] + dex[i + 1:]) == -1, (i, bad)
    for bad in (-1e-9, 1.0 + 1e-9, np.nan):
        assert call(params=dex[:4] + [bad]) == -1
    for ok in (0.0, 1.0):
        assert call(params=dex[:4] + [ok], ws_bytes=0) == -4
    assert call(W=3, H=8, ws_bytes=0) == -1 and call(W=8, H=3, ws_bytes=0) == -1          # H, W < gp_scale: an empty coarse grid
    assert call(W=4, H=4, ws_bytes=0) == -4
    assert call(params=dex[:3] + [0.5, 0.5]) == -1                               # gp_scale < 1
    for model, good in ((2, [1.0, 0.005]), (3, [0.005])):
        assert call(model=model, params=good, ws_bytes=0) == -4
        for i in range(len(good)):
            for bad in (0.0, -1.0, np.nan, np.inf):
                assert call(model=model, params=good[:i] + [bad] + good[i + 1:]) == -1
    assert L.giga_strerror(-1) == b"invalid argument"


# --------------------------------------------------------------------------------------------------------- Python surface
def test_depth_noise_object_and_cpu_tensors():
    d = noise.DepthNoise("dex", seed=3, gp_scale=3)
    assert d.kind == "dex" and d.seed == 3 and d.params == dict(gamma_shape=1000.0, gamma_scale=0.001, gp_sigma=0.005, gp_scale=3.0, gp_rate=0.5)
    assert noise.DepthNoise("trans").params == dict(sigma_p=1.0, sigma_d=0.005) and noise.DepthNoise("norm").params == dict(sigma=0.005)
    assert {k: dict(v) for k, v in noise.PARAMS.items()} == N.DEFAULTS
    with pytest.raises(ValueError):
        noise.DepthNoise("gauss")
    with pytest.raises(TypeError):
        noise.DepthNoise("norm", sigma_p=1)
    with pytest.raises(ValueError):
        noise.DepthNoise("norm", seed=-1)
    img = torch.zeros(2, 4, 4)
    for kind in ("dex", "trans", "norm"):
        with pytest.raises(_capi.GigaHipError):
            noise.DepthNoise(kind).apply(img)
        with pytest.raises(_capi.GigaHipError):
            noise.apply_noise(img, kind)
    with pytest.raises(_capi.GigaHipError):
        noise.DepthNoise("norm").apply(np.zeros((4, 4), F32))
    assert noise.apply_noise(img, "") is img and noise.apply_noise(img, "salt") is img


def _raw_dataset(root, n_scenes, views=3):
    K = perception.CameraIntrinsic(*emu.SMALL_INTRINSIC)
    (root / "scenes").mkdir(parents=True)
    with (root / "setup.json").open("w") as f:
        json.dump({"size": 0.3, "intrinsic": K.to_dict()}, f)
    ids = []
    for s in range(n_scenes):
        ids.append(f"scene{s:02d}")
        np.savez_compressed(root / "scenes" / (ids[-1] + ".npz"), depth_imgs=np.full((views, 37, 53), s, F32), extrinsics=np.zeros((views, 7), F32))
    return ids


def test_construct_dataset_noise_argument_handling(tmp_path, monkeypatch):
    raw = tmp_path / "raw"
    ids = _raw_dataset(raw, 5)
    fused, noised = [], []

    def fake_fuse(size, resolution, depth_batches, intrinsic, extrinsics_batches, device=None):
        fused.append([np.asarray(d) for d in depth_batches])
        B = len(depth_batches)
        return np.zeros((B, resolution, resolution, resolution), F32), [np.zeros((0, 3), F32)] * B

    def fake_noise(nz, depth_batches, image_ids, device=None):
        noised.append((nz, [d.shape for d in depth_batches], list(image_ids)))
        return [np.asarray(d) + 100 for d in depth_batches]

    monkeypatch.setattr(perception, "_fuse_to_host", fake_fuse)
    monkeypatch.setattr(perception, "_noise_scenes", fake_noise)
    nz = noise.DepthNoise("dex", seed=3)
    with pytest.raises(NotImplementedError, match="noise="):
        perception.construct_dataset(raw, tmp_path / "flag", add_noise="dex", noise=nz)
    with pytest.raises(TypeError):
        perception.construct_dataset(raw, tmp_path / "string", noise="dex")
    assert not fused and not noised and not (tmp_path / "flag").exists() and not (tmp_path / "string").exists()
    assert perception.construct_dataset(raw, tmp_path / "a", batch=2, noise=nz) == ids
    assert [c[0] for c in noised] == [nz] * 3 and [c[1] for c in noised] == [[(3, 37, 53)] * 2, [(3, 37, 53)] * 2, [(3, 37, 53)]]
    assert [c[2] for c in noised] == [[(s << 16) | v for s in chunk for v in range(3)] for chunk in ((0, 1), (2, 3), (4,))]
    assert all(np.all(d == 100 + s) for s, d in enumerate(d for call_ in fused for d in call_))         # what is fused is what was noised
    # the ids of a scene do not depend on the batch size
    first = [i for c in noised for i in c[2]]
    noised.clear()
    perception.construct_dataset(raw, tmp_path / "b", batch=32, noise=nz)
    assert len(noised) == 1 and noised[0][2] == first
    # single_view: only the view that is used is noised
    noised.clear(), fused.clear()
    perception.construct_dataset(raw, tmp_path / "c", single_view=True, noise=nz)
    assert noised[0][1] == [(1, 37, 53)] * 5 and noised[0][2] == [s << 16 for s in range(5)] and [d.shape for d in fused[0]] == [(1, 37, 53)] * 5
    # noise=None: nothing is noised, the images arrive as they are in the files
    noised.clear(), fused.clear()
    perception.construct_dataset(raw, tmp_path / "d", noise=None)
    assert not noised and all(np.all(d == s) for s, d in enumerate(fused[0]))
    # 65 536 views have no ids
    many = tmp_path / "many"
    _raw_dataset(many, 1, views=1)
    np.savez_compressed(many / "scenes" / "scene00.npz", depth_imgs=np.zeros((1 << 16, 1, 1), F32), extrinsics=np.zeros((1 << 16, 7), F32))
    noised.clear()
    with pytest.raises(ValueError, match="65 536"):
        perception.construct_dataset(many, tmp_path / "e", noise=nz)
    assert not noised
    perception.construct_dataset(many, tmp_path / "f", single_view=True, noise=nz)
    assert noised[0][2] == [0]
