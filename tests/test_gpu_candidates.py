"""GPU tests of the oriented cloud (giga_tsdf_cloud_emit_oriented) and of giga_grasp_candidates: every output bit for bit against
the numpy restatement (tests/candidates_emu.py), and write_geo_dataset with an executor end to end."""
import functools

import numpy as np
import pytest
import torch

import candidates_emu as cand
import collide_emu as cemu
import tsdf_emu as emu
from candidates_emu import LOWER, UPPER, fake_execute, frame_normals, sampler_cloud
from giga_amd import _capi, candidates, perception, scenes

pytestmark = pytest.mark.gpu
SIZE = 0.3
F32 = np.float32


def dev():
    return torch.device("cuda:0")


def same_bytes(got, want, what, quiet=False):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    word = np.uint32 if want.dtype.itemsize == 4 else np.uint64
    diff = int((np.ascontiguousarray(got).view(word) != np.ascontiguousarray(want).view(word)).sum())
    if diff or not quiet:
        print(f"{what}: {diff} of {want.size} words differ")
    assert diff == 0, what


# ------------------------------------------------------------------------------------------------ oriented emit
def random_volume(R, seed, holes=0.125):
    rng = np.random.default_rng(seed)
    return (rng.random((R, R, R)) * 2 - 1).astype(F32), (rng.random((R, R, R)) >= holes).astype(F32)


def volume_r8():
    """weight-0 cells beside the surface, and a crossing in cell 0 along every axis"""
    t, w = random_volume(8, 8, 0.25)
    t[0, 3, 3], t[1, 3, 3] = 0.4, -0.3
    t[3, 0, 4], t[3, 1, 4] = -0.2, 0.6
    t[5, 5, 0], t[5, 5, 1] = 0.7, -0.1
    for cell in ((0, 3, 3), (1, 3, 3), (3, 0, 4), (3, 1, 4), (5, 5, 0), (5, 5, 1)):
        w[cell] = 1
    w[0, 4, 3] = w[2, 3, 3] = w[3, 0, 5] = w[5, 4, 0] = 0
    return t, w


def synthetic_volume(R, seed, centre_x):
    """the signed distance, in units of 8 voxels, to a ball about a point of the x = centre_x plane; one voxel in eight unobserved"""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(R, dtype=np.float64)] * 3, indexing="ij")
    d = np.sqrt((i - centre_x) ** 2 + (j - R / 2 + 0.3) ** 2 + (k - R / 2 - 0.2) ** 2) - 0.3 * R
    return np.clip(d / 8, -1, 1).astype(F32), (rng.random((R, R, R)) >= 0.125).astype(F32)


@functools.lru_cache(maxsize=None)
def fused_r40():
    """R = 40 fused on the device from six rendered views (the scenes of test_gpu_tsdf_fusion.py); (tsdf, weight) on the host"""
    K = emu.SMALL_INTRINSIC
    ext = emu.six_views(SIZE, 6, 6)
    depth = emu.render_views(emu.make_scene(14), ext, K)
    vol = perception.create_tsdf(SIZE, 40, depth, perception.CameraIntrinsic(*K), ext, dev())
    return vol.state()[0][0].cpu().numpy(), vol.state()[1][0].cpu().numpy()


def oriented(t, w):
    """(points, normals, offsets) of a batch of host volumes, with the points checked against the plain emit"""
    tsdf, weight = torch.from_numpy(np.ascontiguousarray(t)).to(dev()), torch.from_numpy(np.ascontiguousarray(w)).to(dev())
    points, normals, offs = perception.cloud_batch(tsdf, weight, SIZE, normals=True)
    plain, offs2 = perception.cloud_batch(tsdf, weight, SIZE)
    assert torch.equal(points.view(torch.int32), plain.view(torch.int32)) and np.array_equal(offs, offs2)
    assert normals.shape == points.shape and normals.dtype == torch.float32
    return points, normals, offs


@pytest.mark.parametrize("name", ["r4", "r5", "r8-holes-cell0", "r40-fused"])
def test_oriented_cloud_equals_the_restatement(name):
    if name == "r40-fused":
        t, w = fused_r40()
    elif name == "r8-holes-cell0":
        t, w = volume_r8()
    else:
        t, w = random_volume(int(name[1:]), 3, 0.0)
    want_p, want_n = cand.cloud_oriented(t, w, SIZE)
    assert len(want_p) > (0 if t.shape[0] < 8 else 20)
    if name == "r8-holes-cell0":
        v = SIZE / 8
        for axis in range(3):
            assert ((want_p[:, axis] > 0.5 * v) & (want_p[:, axis] < 1.5 * v)).any()
    points, normals, offs = oriented(t[None], w[None])
    assert offs.tolist() == [0, len(want_p)]
    same_bytes(points, want_p, name + " points")
    same_bytes(normals, want_n, name + " normals")
    if name == "r40-fused":
        n = normals.double().cpu().numpy()
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and (n[:, 2] > 0.9).mean() > 0.3       # the table looks up
        vol = perception.TSDFVolume(SIZE, 40, dev())
        vol._tsdf.copy_(torch.from_numpy(t[None]))
        vol._weight.copy_(torch.from_numpy(w[None]))
        p1, n1 = vol.get_cloud(normals=True)
        assert torch.equal(p1, points) and torch.equal(n1, normals) and torch.equal(vol.get_cloud(), points)


def test_oriented_cloud_ragged_batch_with_more_than_1024_workgroup_sums():
    """R = 65: 1073 workgroup sums per scene.  Scene 1 is unobserved; every scene of the batch equals its own call."""
    R = 65
    vols = [synthetic_volume(R, 1, R - 1), synthetic_volume(R, 2, R / 2), synthetic_volume(R, 3, 0)]
    vols[1] = (vols[1][0], np.zeros_like(vols[1][1]))
    t, w = np.stack([v[0] for v in vols]), np.stack([v[1] for v in vols])
    points, normals, offs = oriented(t, w)
    assert offs[1] > 1000 and offs[2] == offs[1] and offs[3] - offs[2] > 1000
    for b in (0, 2):
        want_p, want_n = cand.cloud_oriented(t[b], w[b], SIZE)
        same_bytes(points[offs[b]:offs[b + 1]], want_p, f"R=65 scene {b} points")
        same_bytes(normals[offs[b]:offs[b + 1]], want_n, f"R=65 scene {b} normals")
        p1, n1, _ = oriented(t[b:b + 1], w[b:b + 1])
        assert torch.equal(p1, points[offs[b]:offs[b + 1]]) and torch.equal(n1.view(torch.int32), normals[offs[b]:offs[b + 1]].view(torch.int32))


def test_oriented_cloud_capacity_shortfall():
    t, w = fused_r40()
    tsdf, weight = torch.from_numpy(t[None]).to(dev()), torch.from_numpy(w[None]).to(dev())
    full_p, full_n, offs = perception.cloud_batch(tsdf, weight, SIZE, normals=True)
    total = int(offs[-1])
    assert total > 1000
    L = _capi.lib()
    ws = torch.empty(L.giga_tsdf_cloud_workspace_bytes(1, 40), dtype=torch.uint8, device=dev())
    counts = torch.empty(1, dtype=torch.int32, device=dev())
    _capi.call("giga_tsdf_cloud_count", dev(), tsdf, weight, 1, 40, ws, ws.numel(), counts)
    for cap in (total, 777, 0):
        pts = torch.full((total + 64, 3), -7.0, device=dev())
        nrm = torch.full((total + 64, 3), -7.0, device=dev())
        short = torch.full((1,), -1, dtype=torch.int32, device=dev())
        _capi.call("giga_tsdf_cloud_emit_oriented", dev(), tsdf, weight, 1, 40, SIZE, ws, ws.numel(), pts, nrm, cap, short)
        assert int(short) == total - cap
        assert torch.equal(pts[:cap], full_p[:cap]) and torch.equal(nrm[:cap].view(torch.int32), full_n[:cap].view(torch.int32))
        assert bool((pts[cap:] == -7.0).all()) and bool((nrm[cap:] == -7.0).all())
    p, n, offs2 = perception.cloud_batch(tsdf, weight, SIZE, capacity=100, normals=True)
    assert p.shape == n.shape == (100, 3) and torch.equal(p, full_p[:100]) and np.array_equal(offs, offs2)


# ------------------------------------------------------------------------------------------------ candidates
def scene_cloud(seed, n, E):
    rng = np.random.default_rng(seed)
    return sampler_cloud(rng, n, sorted(rng.choice(n, E, replace=False).tolist()))


def run(clouds, K, Y, seed, ids):
    points = np.concatenate([c[0] for c in clouds]) if clouds else np.zeros((0, 3), F32)
    normals = np.concatenate([c[1] for c in clouds]) if clouds else np.zeros((0, 3), F32)
    offs = np.concatenate(([0], np.cumsum([len(c[0]) for c in clouds])))
    return candidates.grasp_candidates(torch.from_numpy(points).to(dev()), torch.from_numpy(normals).to(dev()), offs, K, lower=LOWER,
                                       upper=UPPER, num_rotations=Y, seed=seed, scene_ids=ids)


def check(got, clouds, K, Y, seed, ids, tag, quiet=False):
    pos, quat, index, counts = got
    assert pos.shape == (len(clouds), K, 3) and quat.shape == (len(clouds), K, Y, 4) and index.shape == (len(clouds), K)
    for b, (p, n) in enumerate(clouds):
        w_pos, w_quat, w_index, E, _ = cand.candidates(p, n, K, LOWER, UPPER, ids[b], seed, Y=Y)
        assert int(counts[b]) == E, (tag, b)
        if E == 0:
            assert not pos[b].any() and not quat[b].any() and not index[b].any()               # left as they were: zeros
            continue
        same_bytes(index[b], w_index, f"{tag} scene {b} index", quiet)
        same_bytes(pos[b], w_pos, f"{tag} scene {b} pos", quiet)
        same_bytes(quat[b], w_quat, f"{tag} scene {b} quat", quiet)


@pytest.mark.parametrize("E, n", [(0, 50), (1, 50), (2, 3), (65, 300), (4097, 9000)])
@pytest.mark.parametrize("K, Y", [(1, 1), (120, 6), (120, 32), (1, 2)])
def test_candidates_equal_the_restatement(E, n, K, Y):
    clouds = [scene_cloud(100 + E, n, E)]
    ids = [0xC0000000 + E]                                                  # above 2^31
    got = run(clouds, K, Y, seed=0x1234567887654321, ids=ids)
    check(got, clouds, K, Y, 0x1234567887654321, ids, f"E={E} K={K} Y={Y}")
    again = run(clouds, K, Y, seed=0x1234567887654321, ids=ids)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_candidates_batch_with_an_empty_scene_and_one_without_eligible_points():
    clouds = [scene_cloud(1, 700, 300), (np.zeros((0, 3), F32), np.zeros((0, 3), F32)), scene_cloud(2, 40, 0), scene_cloud(3, 2100, 1500)]
    ids = [5, 6, 0xFFFFFFFF, 0x80000001]
    got = run(clouds, 120, 6, seed=9, ids=ids)
    assert got[3].tolist() == [300, 0, 0, 1500]
    check(got, clouds, 120, 6, 9, ids, "batch")
    for b in (0, 3):
        one = run(clouds[b:b + 1], 120, 6, seed=9, ids=ids[b:b + 1])
        assert all(torch.equal(x[b], y[0]) for x, y in zip(got, one))
    other = run(clouds, 120, 6, seed=10, ids=ids)
    assert not torch.equal(other[2][0], got[2][0])


def test_candidate_frames_on_the_axes_and_across_the_isclose_switch():
    """one point per scene, so that every candidate of scene b has the normal b: +-x, +-y, +-z, the cosines about the switch of
    np.isclose, and random normals of any length.  A normal with n_z <= -0.1 (-z among them) is not eligible: its scene has no
    candidate."""
    N = frame_normals().astype(F32)
    up = N[:, 2].astype(np.float64) > -0.1
    assert 200 < up.sum() < len(N) and all(up[(N == a).all(1)].all() for a in ([1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 1, 0]))
    assert not up[(N == [0, 0, -1]).all(1)].any()
    c = np.abs(N[:, 0].astype(np.float64)) / np.linalg.norm(N.astype(np.float64), axis=1)
    near = up & (c > 0.9998) & (c < 1)
    assert (near & (np.abs(c - 1) <= 1e-8 + 1e-4)).sum() >= 3 and (near & (np.abs(c - 1) > 1e-8 + 1e-4)).sum() >= 3
    clouds = [(np.array([[0.1, 0.1, 0.1]], F32), N[b:b + 1]) for b in range(len(N))]
    ids = list(range(len(N)))
    got = run(clouds, 2, 6, seed=1, ids=ids)
    assert got[3].tolist() == up.astype(int).tolist()
    check(got, clouds, 2, 6, 1, ids, "frames", quiet=True)


# ------------------------------------------------------------------------------------------------ end to end
def test_write_geo_dataset_with_an_executor_loads_through_the_dataset_reader(tmp_path_factory):
    from giga_amd.dataset import GraspOccDataset
    objects = scenes.ObjectSet(cemu.write_object_set(tmp_path_factory.mktemp("objects") / "set", ("box_a", "box_b", "box_c")))
    base = tmp_path_factory.mktemp("labelled_set")
    raw, root = base / "raw", base / "data"
    calls = []

    def execute(scene, pos, quat, max_opening_width):
        calls.append((scene, pos.shape, quat.shape, max_opening_width))
        return fake_execute(scene, pos, quat, max_opening_width)
    ids, unlabelled = scenes.write_geo_dataset(objects, raw, root, 1, seed=2, batch=1, num_point_per_file=256, num_file=1, device=dev(),
                                               execute=execute, grasps_per_scene=30)
    assert ids == [scenes.scene_id(2, 0)] and unlabelled == [] and calls == [(0, (30, 3), (30, 6, 4), 0.08)]
    ds = GraspOccDataset(str(root), str(raw), num_point_occ=64)
    assert len(ds) == 30 and set(ds.scene_ids) == set(ids) and set(ds.label.tolist()) <= {0, 1} and ds.label.sum() > 0
    hi = 1.1 * 0.05
    lower, upper = candidates.workspace_bounds(0.3, scenes.TABLE_HEIGHT)
    assert (ds._pos >= lower - hi - 1e-6).all() and (ds._pos <= upper + hi + 1e-6).all()
    assert np.abs(np.linalg.norm(ds._quat, axis=1) - 1).max() < 1e-6 and (ds._width > 0).all() and (ds._width <= 0.08).all()
