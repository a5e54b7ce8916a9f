"""GPU tests of the depth noise (csrc/giga_noise.hip: giga_depth_noise through giga_amd.noise) against the reference's own
functions on the same draws (tests/golden/g18_depth_noise.npz) AND against the numpy restatement (tests/noise_emu.py).

Criterion: at most 1 float32 ulp of the expected value per pixel.  Every operation of the kernel is one IEEE rounding that numpy
repeats, except log, cos and sin (and pow), whose last double bits may differ between a device and numpy; such a difference is
about 1e-16 of a noise term below 0.1, far below half a float32 ulp of a depth, so it can move the final float32(...) rounding by
one step at most and can change nothing else.  The rounded source indices of trans are exact: the fixture's tool asserts that no
displaced coordinate lies within 1e-9 of a half-integer."""
import functools
import json

import numpy as np
import pytest
import torch

import noise_emu as N
import render_emu as remu
import tsdf_emu as emu
from giga_amd import _capi, noise, perception, render

pytestmark = pytest.mark.gpu
SIZE = 0.3
F32 = np.float32
SHAPES = N.SMALL_SHAPES + [N.BIG_SHAPE]
KINDS = ("dex", "trans", "norm")


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def g18():
    import os
    return dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_depth_noise.npz")))


@functools.lru_cache(maxsize=None)
def images(shape):
    imgs = N.depth_images(len(N.IDS[shape]), shape[0], shape[1], N.IMAGE_SEED)
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def emulated(kind, shape):
    """the restatement's output for the fixture's images, ids and seed: computed once, shared, never changed"""
    out = N.apply(kind, images(shape), N.IDS[shape], N.FIXTURE_SEED)
    out.setflags(write=False)
    return out


def run(nz, imgs, ids=None):
    src = torch.from_numpy(np.array(imgs, dtype=F32)).to(dev())            # (a copy: the shared inputs are read-only)
    keep = src.clone()
    out = nz.apply(src, ids)
    assert out.is_cuda and out.dtype == torch.float32 and out.shape == src.shape and out.data_ptr() != src.data_ptr()
    assert torch.equal(src, keep), "depth_in was written"
    return out.cpu().numpy()


def within_one_ulp(got, want, what):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / N.ulp32(want)
    print(f"{what}: max {err.max():.3g} ulp, {int((err > 0).sum())} of {err.size} pixels differ")
    assert err.max() <= 1.0, what


def source_indices(nz_params, seed, shape, ids):
    """the (row, column) every trans output pixel was gathered from: an image of its own flat indices (exact in float32 below
    2^24) with a depth noise too small to move them"""
    H, W = shape
    assert H * W < 1 << 24
    index = np.broadcast_to(np.arange(H * W, dtype=F32).reshape(H, W), (len(ids), H, W))
    out = run(noise.DepthNoise("trans", seed, sigma_d=1e-3, **nz_params), index, ids)
    flat = np.rint(out).astype(np.int64)
    assert np.abs(out - flat).max() < 0.1
    return flat // W, flat % W


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_kernel_against_golden_and_emulation(shape):
    H, W = shape
    tag = "%dx%d" % shape
    g, ids, seed = g18(), N.IDS[shape], N.FIXTURE_SEED
    big = shape == N.BIG_SHAPE
    sub = (slice(None), slice(None, None, N.BIG_STRIDE[0]), slice(None, None, N.BIG_STRIDE[1])) if big else (slice(None),) * 3
    on = N.coin(np.array(ids, np.uint64), seed) < 0.5
    assert on.any() and not on.all() and np.array_equal(on, g["dex_on_" + tag])
    for kind in KINDS:
        got = run(noise.DepthNoise(kind, seed), images(shape), ids)
        within_one_ulp(got, emulated(kind, shape), f"{kind} {tag} against the restatement")
        within_one_ulp(got[sub], g[kind + "_" + tag], f"{kind} {tag} against the reference's function")
        if big:
            sums = got.astype(np.float64).sum(axis=(1, 2))
            print(kind, "sums", sums, g[kind + "_sum_" + tag])
            assert np.all(np.abs(sums - g[kind + "_sum_" + tag]) <= H * W * 2.0 ** -22)          # a ulp of a value below 4, per pixel
        assert not np.array_equal(got, images(shape))
    r, c = source_indices({}, seed, shape, ids)
    for i, image_id in enumerate(ids):
        _, _, er, ec = N.trans_coords(H, W, image_id, seed)
        assert np.array_equal(r[i], er) and np.array_equal(c[i], ec), (tag, image_id)
        assert np.array_equal(r[i][sub[1:]], g["r_" + tag][i]) and np.array_equal(c[i][sub[1:]], g["c_" + tag][i])
    if shape == (65, 130):
        assert (r != np.arange(H)[None, :, None]).any() and (r[:, 32, :] < 32).any() and (c[:, :, 128] < 128).any()     # gathers across tiles


@pytest.mark.parametrize("shape", [(30, 45), (65, 130)], ids=lambda s: "%dx%d" % s)
def test_non_default_parameters(shape):
    H, W = shape
    ids, seed = [5, 6, (1 << 33) + 1], 4
    imgs = N.depth_images(3, H, W, 9)
    for params in (dict(gp_scale=3, gp_rate=1.0), dict(gp_rate=0.0), dict(gamma_shape=0.5, gamma_scale=2.0, gp_sigma=0.02, gp_rate=1.0),
                   dict(gamma_shape=3.0, gamma_scale=0.3, gp_scale=2.5)):
        got = run(noise.DepthNoise("dex", seed, **params), imgs, ids)
        within_one_ulp(got, N.apply("dex", imgs, ids, seed, **params), f"dex {params}")
    assert N.coarse_shape(H, W, 3) != N.coarse_shape(H, W, 4)
    for sigma_p in (2.5, 0.3):
        for image_id in ids:
            fr, fc, _, _ = N.trans_coords(H, W, image_id, seed, sigma_p)
            for v in (fr, fc):
                assert np.abs(np.abs(v - np.floor(v)) - 0.5).min() > 1e-9          # the rounding cannot depend on the last bits
        got = run(noise.DepthNoise("trans", seed, sigma_p=sigma_p, sigma_d=0.02), imgs, ids)
        within_one_ulp(got, N.apply("trans", imgs, ids, seed, sigma_p=sigma_p, sigma_d=0.02), f"trans sigma_p {sigma_p}")
        r, c = source_indices(dict(sigma_p=sigma_p), seed, shape, ids)
        for i, image_id in enumerate(ids):
            _, _, er, ec = N.trans_coords(H, W, image_id, seed, sigma_p)
            assert np.array_equal(r[i], er) and np.array_equal(c[i], ec)
    got = run(noise.DepthNoise("norm", seed, sigma=0.05), imgs, ids)
    within_one_ulp(got, N.apply("norm", imgs, ids, seed, sigma=0.05), "norm sigma 0.05")


@pytest.mark.parametrize("kind", KINDS)
def test_batch_invariance_determinism_and_seeds(kind):
    H, W = 65, 130
    ids = [7, 0, (1 << 40) + 3, 7, 1]
    imgs = N.depth_images(5, H, W, 21).copy()
    imgs[3] = imgs[0]
    nz = noise.DepthNoise(kind, seed=11)
    batch = run(nz, imgs, ids)
    for i, image_id in enumerate(ids):
        single = run(nz, imgs[i:i + 1], [image_id])
        assert np.array_equal(single[0].view(np.uint32), batch[i].view(np.uint32)), (kind, i)
        assert np.array_equal(run(nz, imgs[i], [image_id]).view(np.uint32), batch[i].view(np.uint32))          # an (H, W) tensor
    assert np.array_equal(batch[0].view(np.uint32), batch[3].view(np.uint32))
    assert not np.array_equal(batch[0], batch[1]) and not np.array_equal(run(nz, imgs[:1], [1])[0], batch[0])
    assert np.array_equal(run(nz, imgs, ids).view(np.uint32), batch.view(np.uint32))
    assert np.array_equal(run(nz, imgs[:2])[1].view(np.uint32), run(nz, imgs[1:2], [1])[0].view(np.uint32))   # default ids 0 .. n-1
    other = run(noise.DepthNoise(kind, seed=12), imgs, ids)
    assert (other != batch).mean() > 0.9
    high = run(noise.DepthNoise(kind, seed=11 + (1 << 32)), imgs, ids)                                        # the key's high word
    assert (high != batch).mean() > 0.9
    assert np.array_equal(noise.apply_noise(torch.from_numpy(imgs).to(dev()), kind, 11, ids).cpu().numpy().view(np.uint32),
                          run(noise.DepthNoise(kind, 11), imgs, ids).view(np.uint32))


def test_unaligned_views_and_other_dtypes():
    """a view that starts 4 bytes into an allocation (no 16-byte accesses possible) and a float64 tensor give the same bytes"""
    H, W = 24, 36
    imgs = N.depth_images(2, H, W, 3)
    for kind in KINDS:
        nz = noise.DepthNoise(kind, seed=2)
        want = run(nz, imgs)
        flat = torch.zeros(imgs.size + 1, device=dev())
        flat[1:] = torch.from_numpy(imgs.reshape(-1)).to(dev())
        view = flat[1:].reshape(2, H, W)
        assert view.data_ptr() % 16 == 4
        assert np.array_equal(nz.apply(view).cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert np.array_equal(nz.apply(torch.from_numpy(imgs.astype(np.float64)).to(dev())).cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert noise.DepthNoise("norm").apply(torch.zeros(0, 4, 4, device=dev())).shape == (0, 4, 4)
    with pytest.raises(_capi.GigaHipError):
        noise.DepthNoise("dex").apply(torch.zeros(1, 3, 8, device=dev()))          # H < gp_scale


# ----------------------------------------------------------------------------------------------------------- end to end
def _raw_dataset(root, n_scenes, views=3):
    from scipy.spatial.transform import Rotation
    K = perception.CameraIntrinsic(*emu.SMALL_INTRINSIC)
    (root / "scenes").mkdir(parents=True)
    with (root / "setup.json").open("w") as f:
        json.dump({"size": SIZE, "intrinsic": K.to_dict()}, f)
    scenes = {}
    for s in range(n_scenes):
        ext = emu.six_views(SIZE, views, 6)
        depth = emu.render_views(emu.make_scene(100 + s), ext, emu.SMALL_INTRINSIC)
        poses = np.stack([np.r_[Rotation.from_matrix(E[:3, :3]).as_quat(), E[:3, 3]] for E in ext])
        np.savez_compressed(root / "scenes" / (f"scene{s:02d}.npz"), depth_imgs=depth, extrinsics=poses)
        scenes[f"scene{s:02d}"] = (depth, poses)
    return K, scenes


def _files(root):
    return {p.relative_to(root).as_posix(): dict(np.load(p)) for p in sorted(root.rglob("*.npz"))}


def _same_files(a, b):
    assert sorted(a) == sorted(b) and len(a) == 4
    for name in a:
        assert sorted(a[name]) == sorted(b[name])
        for k in a[name]:
            assert a[name][k].dtype == b[name][k].dtype and np.array_equal(a[name][k], b[name][k]), (name, k)


def test_construct_dataset_with_noise(tmp_path):
    raw = tmp_path / "raw"
    K, scenes = _raw_dataset(raw, 2)
    nz = noise.DepthNoise("dex", seed=3)
    assert perception.construct_dataset(raw, tmp_path / "noised", resolution=16, device=dev(), noise=nz) == sorted(scenes)
    perception.construct_dataset(raw, tmp_path / "plain", resolution=16, device=dev())
    perception.construct_dataset(raw, tmp_path / "none", resolution=16, device=dev(), noise=None)
    perception.construct_dataset(raw, tmp_path / "single", resolution=16, device=dev(), noise=nz, single_view=True, batch=1)
    noised, plain = _files(tmp_path / "noised"), _files(tmp_path / "plain")
    _same_files(plain, _files(tmp_path / "none"))
    noisy_depth = [nz.apply(torch.from_numpy(d).to(dev()), [(s << 16) | v for v in range(len(d))]) for s, (d, _) in enumerate(scenes.values())]
    poses = [p for _, p in scenes.values()]
    want = perception.create_tsdfs(SIZE, 16, noisy_depth, K, poses, dev()).cpu().numpy()
    clean = perception.create_tsdfs(SIZE, 16, [d for d, _ in scenes.values()], K, poses, dev()).cpu().numpy()
    one = perception.create_tsdfs(SIZE, 16, [d[:1] for d in noisy_depth], K, [p[:1] for p in poses], dev()).cpu().numpy()
    single = _files(tmp_path / "single")
    for s, sid in enumerate(sorted(scenes)):
        got = noised[f"scenes/{sid}.npz"]["grid"]
        assert got.shape == (1, 16, 16, 16) and np.array_equal(got[0].view(np.uint32), want[s].view(np.uint32))
        assert np.array_equal(plain[f"scenes/{sid}.npz"]["grid"][0].view(np.uint32), clean[s].view(np.uint32))
        assert (got[0] != clean[s]).sum() > 50
        assert np.array_equal(single[f"scenes/{sid}.npz"]["grid"][0].view(np.uint32), one[s].view(np.uint32))
    with pytest.raises(NotImplementedError):
        perception.construct_dataset(raw, tmp_path / "flag", add_noise="dex", device=dev())


def test_acquire_tsdf_with_noise_feeds_both_volumes_the_same_images():
    v, f = remu.scene_to_mesh(emu.make_scene(0))
    nz = noise.DepthNoise("dex", seed=5)
    vol, pc, _ = render.acquire_tsdf(v, f, 2, N=6, resolution=16, device=dev(), noise=nz)
    intr, ext = render.sim_intrinsic(), render.acquire_extrinsics(2, 6, SIZE)
    depth = render.render_depth(v, f, intr, ext, device=dev())
    noisy = nz.apply(depth)
    assert not torch.equal(noisy, depth)
    assert torch.equal(vol.grid(), perception.create_tsdf(SIZE, 16, noisy, intr, ext, dev()).grid())
    assert torch.equal(pc, perception.create_tsdf(SIZE, 120, noisy, intr, ext, dev()).get_cloud()) and len(pc) > 1000
    plain, pc_plain, _ = render.acquire_tsdf(v, f, 2, N=6, resolution=16, device=dev())
    assert torch.equal(plain.grid(), perception.create_tsdf(SIZE, 16, depth, intr, ext, dev()).grid())
    assert not torch.equal(plain.grid(), vol.grid()) and not (len(pc) == len(pc_plain) and torch.equal(pc, pc_plain))
    # the batched form: view k of mesh b has the id (b << 16) | k
    meshes = [(v, f), remu.scene_to_mesh(emu.make_scene(1))]
    grids = render.acquire_tsdfs(meshes, 2, N=6, resolution=16, device=dev(), noise=nz)
    for b, (mv, mf) in enumerate(meshes):
        d = nz.apply(render.render_depth(mv, mf, intr, ext, device=dev()), [(b << 16) | k for k in range(2)])
        assert torch.equal(grids[b], perception.create_tsdf(SIZE, 16, d, intr, ext, dev()).grid()[0])
    assert torch.equal(grids[0], vol.grid()[0])
    assert torch.equal(render.acquire_tsdfs(meshes, 2, N=6, resolution=16, device=dev()),
                       render.acquire_tsdfs(meshes, 2, N=6, resolution=16, device=dev(), noise=None))


def test_plan_from_depth_with_noise(sd7):
    from giga_amd import networks
    from giga_amd.detection import VGNImplicit
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    planner = VGNImplicit(None, "giga", net=net.to(dev()).eval(), best=True, force_detection=True, qual_th=0.6, out_th=0.1)
    K = emu.SMALL_INTRINSIC
    intr = perception.CameraIntrinsic(*K)
    ext = emu.six_views(SIZE, 6, 6)
    depth = emu.render_views(emu.make_scene(70), ext, K)
    nz = noise.DepthNoise("norm", seed=1)
    a = planner.plan_from_depth(depth, intr, ext, size=SIZE, noise=nz)
    b = planner.plan_from_depth(nz.apply(torch.from_numpy(depth).to(dev())), intr, ext, size=SIZE)
    assert len(a[0]) == len(b[0]) and np.array_equal(a[1], b[1])
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x["rotation"], y["rotation"]) and np.array_equal(x["translation"], y["translation"]) and x["width"] == y["width"]
