"""GPU tests of the depth fusion (csrc/giga_tsdf.hip: giga_tsdf_integrate, giga_tsdf_cloud_count / _emit) against the numpy
restatement of tests/tsdf_emu.py: grid, state and cloud are compared BYTE FOR BYTE (every operation of the kernel is one IEEE
rounding in the precision the header states), on images rendered analytically from seeds."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tsdf_emu as emu
from giga_amd import _capi, perception

pytestmark = pytest.mark.gpu
SIZE = 0.3
F32 = np.float32


def dev():
    return torch.device("cuda:0")


def intrinsic_of(K):
    return perception.CameraIntrinsic(*K)


@functools.lru_cache(maxsize=None)
def views(seed, K, n=6, N=6):
    """(depth (n, H, W), extrinsics (n, 4, 4)) of scene `seed`: the first n of N cameras of the reference's circle."""
    ext = emu.six_views(SIZE, n, N)
    return emu.render_views(emu.make_scene(seed), ext, K), ext


def same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{what}: {diff} of {want.size} words differ")
    assert diff == 0, what


def check_scene(tsdf, weight, grid, cloud, depth, ext, K, R, tag):
    stats = {}
    t, w, g = emu.fuse(depth, ext, K[2:], SIZE, R, stats=stats)
    print(f"{tag}: {stats.get('knife_edge', 0)} knife-edge of {stats.get('voxel_views', 0)} voxel-views; "
          f"{int((w != 0).sum())} voxels observed, {int((g != 0).sum())} in the grid")
    same_bytes(weight, w, tag + " weight")
    same_bytes(tsdf, t, tag + " tsdf")
    same_bytes(grid, g, tag + " grid")
    same_bytes(cloud, emu.cloud(t, w, SIZE), tag + " cloud")
    return t, w, g


@pytest.mark.parametrize("R, K, n, seed", [(40, emu.SIM_INTRINSIC, 6, 11), (40, emu.SIM_INTRINSIC, 1, 12), (120, emu.SIM_INTRINSIC, 6, 13),
                                           (40, emu.SMALL_INTRINSIC, 6, 14), (40, emu.SMALL_INTRINSIC, 1, 15), (120, emu.SMALL_INTRINSIC, 6, 16)],
                         ids=["r40-six-480x640", "r40-one-480x640", "r120-six-480x640", "r40-six-37x53", "r40-one-37x53", "r120-six-37x53"])
def test_create_tsdf_matches_the_restatement_byte_for_byte(R, K, n, seed):
    depth, ext = views(seed, K, n, 6)
    assert (depth > 0).mean() > 0.5
    vol = perception.create_tsdf(SIZE, R, depth, intrinsic_of(K), ext, dev())
    assert (vol.size, vol.resolution, vol.voxel_size, vol.sdf_trunc) == (SIZE, R, SIZE / R, 4 * (SIZE / R))
    tsdf, weight = vol.state()
    g = vol.grid()
    assert g.is_cuda and g.shape == (1, R, R, R)
    host = vol.get_grid()
    assert isinstance(host, np.ndarray) and host.shape == (1, R, R, R) and np.array_equal(host, g.cpu().numpy())
    cloud = vol.get_cloud()
    assert cloud.is_cuda and cloud.shape[1] == 3 and len(cloud) > 100
    check_scene(tsdf[0], weight[0], g[0], cloud, depth, ext, K, R, f"R={R} {n} views {K[1]}x{K[0]}")


def test_ragged_batch_equals_the_restatement_and_single_scene_calls():
    K = emu.SMALL_INTRINSIC
    counts = (6, 1, 3, 0)
    scenes = [views(20 + b, K, n, 6) if n else (np.zeros((0, K[1], K[0]), F32), np.zeros((0, 4, 4))) for b, n in enumerate(counts)]
    tsdf, weight, grid = perception.fuse_scenes(SIZE, 40, [s[0] for s in scenes], intrinsic_of(K), [s[1] for s in scenes], dev())
    grid2 = perception.create_tsdfs(SIZE, 40, [s[0] for s in scenes], intrinsic_of(K), [s[1] for s in scenes], dev())
    assert grid2.is_cuda and grid2.shape == (4, 40, 40, 40) and torch.equal(grid, grid2)                    # two runs, same bytes
    points, offs = perception.cloud_batch(tsdf, weight, SIZE)
    assert offs[0] == 0 and offs[-1] == len(points) and offs[4] == offs[3]
    for b, (depth, ext) in enumerate(scenes):
        check_scene(tsdf[b], weight[b], grid[b], points[offs[b]:offs[b + 1]], depth, ext, K, 40, f"batch scene {b} ({counts[b]} views)")
        one = perception.create_tsdf(SIZE, 40, depth, intrinsic_of(K), ext, dev())
        assert torch.equal(one.grid()[0], grid[b]) and torch.equal(one.state()[0][0], tsdf[b]) and torch.equal(one.state()[1][0], weight[b])
        assert torch.equal(one.get_cloud(), points[offs[b]:offs[b + 1]])
    assert not grid[3].any() and not weight[3].any()


def test_ragged_batch_at_the_camera_resolution():
    K = emu.SIM_INTRINSIC
    counts = (2, 0, 1)
    scenes = [views(30 + b, K, n, 6) if n else (np.zeros((0, K[1], K[0]), F32), np.zeros((0, 4, 4))) for b, n in enumerate(counts)]
    tsdf, weight, grid = perception.fuse_scenes(SIZE, 40, [s[0] for s in scenes], intrinsic_of(K), [s[1] for s in scenes], dev())
    points, offs = perception.cloud_batch(tsdf, weight, SIZE)
    for b, (depth, ext) in enumerate(scenes):
        check_scene(tsdf[b], weight[b], grid[b], points[offs[b]:offs[b + 1]], depth, ext, K, 40, f"480x640 batch scene {b}")


def test_all_zero_depth_images():
    K = emu.SMALL_INTRINSIC
    depth, ext = views(40, K, 3, 6)
    zero = np.zeros_like(depth)
    vol = perception.create_tsdf(SIZE, 40, zero, intrinsic_of(K), ext, dev())
    assert not vol.grid().any() and not vol.state()[0].any() and not vol.state()[1].any() and vol.get_cloud().shape == (0, 3)
    mixed = depth.copy()
    mixed[1] = 0
    vol = perception.create_tsdf(SIZE, 40, mixed, intrinsic_of(K), ext, dev())
    check_scene(vol.state()[0][0], vol.state()[1][0], vol.grid()[0], vol.get_cloud(), mixed, ext, K, 40, "middle view empty")
    # an empty view changes nothing: the volume equals the one of the two other views
    two = perception.create_tsdf(SIZE, 40, depth[[0, 2]], intrinsic_of(K), ext[[0, 2]], dev())
    assert torch.equal(two.grid(), vol.grid()) and torch.equal(two.state()[1], vol.state()[1])


def test_incremental_integration_equals_one_call_and_repeats():
    K = emu.SMALL_INTRINSIC
    depth, ext = views(41, K, 6, 6)
    intr = intrinsic_of(K)
    whole = perception.create_tsdf(SIZE, 40, depth, intr, ext, dev())
    again = perception.create_tsdf(SIZE, 40, depth, intr, ext, dev())
    step = perception.TSDFVolume(SIZE, 40, dev())
    from scipy.spatial.transform import Rotation
    for k in range(6):
        # one view per call, the extrinsic in a different form each time
        form = (ext[k], ext[k].tolist(), SimpleNamespace(as_matrix=lambda k=k: ext[k]))[k % 3]
        step.integrate(depth[k], intr, form)
    for a, b in zip((whole.grid(), *whole.state(), whole.get_cloud()), (step.grid(), *step.state(), step.get_cloud())):
        assert torch.equal(a, b)
    for a, b in zip((whole.grid(), *whole.state(), whole.get_cloud()), (again.grid(), *again.state(), again.get_cloud())):
        assert torch.equal(a, b)
    # a pose list (the raw dataset's form) gives the volume of its matrix
    poses = np.stack([np.r_[Rotation.from_matrix(E[:3, :3]).as_quat(), E[:3, 3]] for E in ext])
    mats = np.stack([perception.extrinsic_matrix(p) for p in poses])
    a = perception.create_tsdf(SIZE, 40, depth, intr, poses, dev())
    b = perception.create_tsdf(SIZE, 40, depth, intr, mats, dev())
    assert torch.equal(a.grid(), b.grid())
    check_scene(a.state()[0][0], a.state()[1][0], a.grid()[0], a.get_cloud(), depth, mats, K, 40, "pose lists")


def test_cloud_capacity_shortfall_is_reported_and_respected():
    K = emu.SMALL_INTRINSIC
    scenes = [views(50 + b, K, 3, 6) for b in range(2)]
    tsdf, weight, _ = perception.fuse_scenes(SIZE, 40, [s[0] for s in scenes], intrinsic_of(K), [s[1] for s in scenes], dev())
    full, offs = perception.cloud_batch(tsdf, weight, SIZE)
    total = int(offs[-1])
    assert total > 1000 and offs[1] > 0 and offs[2] > offs[1]
    L = _capi.lib()
    ws = torch.empty(L.giga_tsdf_cloud_workspace_bytes(2, 40), dtype=torch.uint8, device=dev())
    counts = torch.empty(2, dtype=torch.int32, device=dev())
    for cap in (total, int(offs[1]) + 7, 5, 0):
        buf = torch.full((total + 64, 3), -7.0, device=dev())
        short = torch.full((1,), -1, dtype=torch.int32, device=dev())
        with torch.cuda.device(dev()):
            _capi.check(L.giga_tsdf_cloud_count(_capi.ptr(tsdf), _capi.ptr(weight), 2, 40, _capi.ptr(ws), ws.numel(), _capi.ptr(counts),
                                                _capi.stream_ptr(dev())), "count")
            _capi.check(L.giga_tsdf_cloud_emit(_capi.ptr(tsdf), _capi.ptr(weight), 2, 40, SIZE, _capi.ptr(ws), ws.numel(), _capi.ptr(buf),
                                               cap, _capi.ptr(short), _capi.stream_ptr(dev())), "emit")
        assert counts.tolist() == [int(offs[1]), int(offs[2] - offs[1])]
        assert int(short) == total - cap
        assert torch.equal(buf[:cap], full[:cap]) and bool((buf[cap:] == -7.0).all())
    part, offs2 = perception.cloud_batch(tsdf, weight, SIZE, capacity=100)
    assert part.shape == (100, 3) and torch.equal(part, full[:100]) and np.array_equal(offs, offs2)


def synthetic_volume(R, seed):
    """(tsdf, weight) without any integration: the signed distance, in units of 8 voxels, to a ball about the middle of the
    x = R - 1 face, so that the cells with the highest numbers hold crossings too; one voxel in eight unobserved."""
    rng = np.random.default_rng(seed)
    i, j, k = np.meshgrid(*[np.arange(R, dtype=np.float64)] * 3, indexing="ij")
    d = np.sqrt((i - (R - 1)) ** 2 + (j - R / 2 + 0.3) ** 2 + (k - R / 2 - 0.2) ** 2) - 0.3 * R
    return np.clip(d / 8, -1, 1).astype(F32), (rng.random((R, R, R)) >= 0.125).astype(F32)


@pytest.mark.parametrize("R, nblk", [(64, 1024), (65, 1073)], ids=["one-full-round", "second-round"])
def test_cloud_of_a_synthetic_volume_with_a_thousand_workgroup_sums(R, nblk):
    """The scan of a scene's workgroup sums runs in rounds of 1024: exactly one full round, and 49 sums into a second one."""
    assert -(-R ** 3 // 256) == nblk
    t, w = synthetic_volume(R, R)
    want = emu.cloud(t, w, SIZE)
    far = want[:, 0] > (R - 3) * (SIZE / R)                   # points of the last three x-planes: the last 49 workgroups and more
    assert 1000 < len(want) < 20000 and far.sum() > 50 and far[-1]
    points, offs = perception.cloud_batch(torch.from_numpy(t[None]).to(dev()), torch.from_numpy(w[None]).to(dev()), SIZE)
    assert offs.tolist() == [0, len(want)]
    same_bytes(points, want, f"synthetic R={R} cloud")


def test_cloud_bases_over_more_than_a_wave_of_scenes():
    """65 scenes at R = 4, every fourth one unobserved: the bases of the scenes are taken 64 at a time, scene 64 in a second
    round."""
    rng = np.random.default_rng(4)
    t = (rng.random((65, 4, 4, 4)) * 2 - 1).astype(F32)
    w = (rng.random((65, 4, 4, 4)) >= 0.125).astype(F32)
    w[1::4] = 0
    want = [emu.cloud(t[b], w[b], SIZE) for b in range(65)]
    assert all(len(c) == 0 for c in want[1::4]) and len(want[63]) > 0 and len(want[64]) > 0
    points, offs = perception.cloud_batch(torch.from_numpy(t).to(dev()), torch.from_numpy(w).to(dev()), SIZE)
    assert np.array_equal(np.diff(offs), [len(c) for c in want])
    same_bytes(points, np.concatenate(want), "65 scenes cloud")


def test_dense_grids_reproduces_the_new_export():
    K = emu.SMALL_INTRINSIC
    scenes = [views(60 + b, K, 2 + b, 6) for b in range(3)]
    grid = perception.create_tsdfs(SIZE, 40, [s[0] for s in scenes], intrinsic_of(K), [s[1] for s in scenes], dev())
    sparse = []
    for b in range(3):
        idx = torch.nonzero(grid[b])
        assert len(idx) > 1000
        sparse.append((idx.to(torch.int32), grid[b][idx[:, 0], idx[:, 1], idx[:, 2]]))
    assert torch.equal(perception.dense_grids(sparse, 40, dev()), grid)


def _net(sd7):
    from giga_amd import networks
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    return net.to(dev()).eval()


def _same_plan(a, b):
    (ga, sa, _), (gb, sb, _) = a, b
    assert len(ga) == len(gb) and np.array_equal(sa, sb)
    for x, y in zip(ga, gb):
        assert np.array_equal(x["rotation"], y["rotation"]) and np.array_equal(x["translation"], y["translation"]) and x["width"] == y["width"]


def test_planner_takes_the_device_volume_and_plans_from_depth(sd7):
    from giga_amd.detection import VGNImplicit
    K = emu.SMALL_INTRINSIC
    intr = intrinsic_of(K)
    planner = VGNImplicit(None, "giga", net=_net(sd7), best=True, force_detection=True, qual_th=0.6, out_th=0.1)
    found = 0
    for seed in (70, 71, 72, 73):
        depth, ext = views(seed, K, 6, 6)
        vol = perception.create_tsdf(SIZE, 40, depth, intr, ext, dev())
        on_device = planner(SimpleNamespace(tsdf=vol))
        found += len(on_device[0])
        print(f"scene {seed}: {len(on_device[0])} grasps")
        _same_plan(on_device, planner(SimpleNamespace(tsdf=vol.get_grid())))
        _same_plan(on_device, planner.plan_from_depth(depth, intr, ext, size=SIZE))
        # a separate volume for the post-processing (the reference's state carries a second volume with its own voxel_size)
        other = perception.create_tsdf(SIZE, 40, depth[:3], intr, ext[:3], dev())
        a = planner(SimpleNamespace(tsdf=vol, tsdf_process=other))
        host = SimpleNamespace(get_grid=vol.get_grid, voxel_size=vol.voxel_size, size=vol.size)
        host_p = SimpleNamespace(get_grid=other.get_grid, voxel_size=other.voxel_size, size=other.size)
        _same_plan(a, planner(SimpleNamespace(tsdf=host, tsdf_process=host_p)))
    assert found > 0                                      # the comparison is not about empty plans


def test_construct_dataset_output_loads_through_the_dataset_reader(tmp_path):
    import json

    from scipy.spatial.transform import Rotation

    from giga_amd import dataset, synth
    raw, out = tmp_path / "raw", tmp_path / "data"
    synth.write_training_set(str(tmp_path / "unused"), str(raw), n_scenes=3, grasps_per_scene=2, seed=3)
    with (raw / "setup.json").open() as f:
        intr = perception.CameraIntrinsic.from_dict(json.load(f)["intrinsic"])
    K = (intr.width, intr.height, float(intr.fx), float(intr.fy), float(intr.cx), float(intr.cy))
    assert K == emu.SIM_INTRINSIC
    ids = sorted(p.name for p in (raw / "occ").iterdir())
    (raw / "scenes").mkdir()
    want = {}
    for s, sid in enumerate(ids):
        depth, ext = views(80 + s, K, 2, 6)
        poses = np.stack([np.r_[Rotation.from_matrix(E[:3, :3]).as_quat(), E[:3, 3]] for E in ext])
        np.savez_compressed(raw / "scenes" / (sid + ".npz"), depth_imgs=depth, extrinsics=poses)
        want[sid] = (depth, np.stack([perception.extrinsic_matrix(p) for p in poses]))
    assert perception.construct_dataset(raw, out, batch=2, device=dev()) == ids
    ds = dataset.GraspOccDataset(str(out), str(raw), num_point_occ=32)
    assert len(ds) == 6
    for sid, (depth, ext) in want.items():
        t, w, g = emu.fuse(depth, ext, K[2:], SIZE, 40)
        got = dataset.read_voxel_grid(out, sid)
        assert got.shape == (1, 40, 40, 40) and got.dtype == F32 and np.array_equal(got[0].view(np.uint32), g.view(np.uint32))
        assert np.array_equal(ds.grid(sid), got)
        pc = np.load(out / "point_clouds" / (sid + ".npz"))["pc"]
        full = emu.cloud(t, w, SIZE)
        keep = np.all((full >= perception.CLOUD_LOWER) & (full <= perception.CLOUD_UPPER), axis=1)
        assert 0 < len(pc) < len(full) and np.array_equal(pc, full[keep].astype(np.float64))
    x = ds.item(0)[0]
    assert x.shape == (40, 40, 40) and x.dtype == F32
    single = tmp_path / "single"
    perception.construct_dataset(raw, single, single_view=True, device=dev())
    depth, ext = want[ids[0]]
    assert np.array_equal(dataset.read_voxel_grid(single, ids[0])[0], emu.fuse(depth[:1], ext[:1], K[2:], SIZE, 40)[2])
