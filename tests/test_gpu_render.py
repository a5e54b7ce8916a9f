"""GPU tests of the depth renderer (csrc/giga_render.hip: giga_depth_render) and of what giga_amd.render builds on it.  Images are
compared BYTE FOR BYTE with the numpy restatement of tests/render_emu.py (every operation of the kernel is one IEEE rounding in
double); the closed loop mesh -> images -> volume is compared byte for byte with tests/tsdf_emu.fuse on the restatement's images."""
import functools
import json
import shutil

import numpy as np
import pytest
import torch

import render_emu as remu
import tsdf_emu as emu
from giga_amd import _capi, perception, render

pytestmark = pytest.mark.gpu
SIZE = 0.3
F32 = np.float32
FAR = 2.0
CHUNK = 256                                   # triangles the kernel's workgroup takes per step (RENDER_BLOCK); its LDS list holds 384
PIXEL_CAM = (32, 16, 64.0, 64.0, 16.0, 8.0)
ODD_CAM = (101, 67, 90.0, 88.0, 50.25, 33.5)  # no multiple of the 16 x 16 tile


def dev():
    return torch.device("cuda:0")


def intrinsic_of(K):
    return perception.CameraIntrinsic(*K)


def scene_mesh(seed):
    return remu.scene_to_mesh(emu.make_scene(seed))


@functools.lru_cache(maxsize=None)
def sim_reference():
    """the restatement's six 480x640 images of scene 0 (plane + 2 boxes, 26 triangles): computed once, shared, never changed"""
    v, f = scene_mesh(0)
    assert len(f) == 26
    imgs = remu.render_views(v, f, emu.six_views(SIZE), emu.SIM_INTRINSIC)
    imgs.setflags(write=False)
    return imgs


def same_bytes(got, want, what):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
    print(f"{what}: {diff} of {want.size} words differ; {int((want != F32(FAR)).sum())} pixels hit")
    assert diff == 0, what


def watertight_square(flip):
    return remu.grid_square((4 - 16) / 128.0, (2 - 8) / 128.0, 2 / 128.0, 12, 6, 0.5, flip)


def _nan_and_bad_index():
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    v = np.concatenate([v, [[np.nan, 0, 0.4], [0.1, 0.1, 0.4], [-0.1, 0.1, 0.4], [np.inf, 0.0, 0.3]]]).astype(F32)
    f = np.concatenate([f, [[4, 5, 6]], [[0, 1, 8]], [[0, -1, 2]], [[7, 5, 6]]]).astype(np.int32)
    return v, f


BEHIND = (np.array([[-1, 0.0625, 2], [1, 0.0625, 2], [0, 0.0625, -1]], F32), np.array([[0, 1, 2]], np.int32))
EMPTY = (np.zeros((0, 3), F32), np.zeros((0, 3), np.int32))
CASES = {
    "six-37x53-plane-boxes": lambda: (scene_mesh(0), emu.SMALL_INTRINSIC, emu.six_views(SIZE), {}),
    "one-37x53-icosphere-1280": lambda: (remu.icosphere((0.15, 0.15, 0.1), 0.06, 3), emu.SMALL_INTRINSIC, emu.six_views(SIZE, 1, 6), {}),
    "two-67x101-plane-box": lambda: (scene_mesh(2), ODD_CAM, emu.six_views(SIZE, 2, 6), {}),
    "watertight": lambda: (watertight_square(False), PIXEL_CAM, np.eye(4)[None], {}),
    "watertight-flipped": lambda: (watertight_square(True), PIXEL_CAM, np.eye(4)[None], {}),
    "behind-the-camera": lambda: (BEHIND, PIXEL_CAM, np.eye(4)[None], {}),
    "empty-mesh": lambda: (EMPTY, PIXEL_CAM, np.eye(4)[None], {}),
    "nan-vertex-bad-index": lambda: (_nan_and_bad_index(), PIXEL_CAM, np.eye(4)[None], {}),
    "pixel-offset-half": lambda: (scene_mesh(3), emu.SMALL_INTRINSIC, emu.six_views(SIZE, 2, 6), dict(pixel_offset=0.5)),
    "near-far": lambda: (remu.box_mesh((-0.05, -0.05, 0.05), (0.05, 0.05, 0.3)), PIXEL_CAM, np.eye(4)[None], dict(near=0.1, far=0.25)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_render_depth_matches_the_restatement_byte_for_byte(case):
    (v, f), K, ext, kw = CASES[case]()
    if case == "one-37x53-icosphere-1280":
        assert len(f) == 1280 > 2 * CHUNK                                # several steps and more than one flush of the LDS list
    want = remu.render_views(v, f, ext, K, kw.get("near", 0.1), kw.get("far", FAR), kw.get("pixel_offset", 0.0))
    got = render.render_depth(v, f, intrinsic_of(K), ext, device=dev(), **kw)
    assert got.is_cuda and got.shape == (len(ext), K[1], K[0])
    same_bytes(got, want, case)
    if case.startswith("watertight"):
        inside = np.zeros((16, 32), bool)
        inside[2:15, 4:29] = True
        g = got[0].cpu().numpy()
        assert (g[inside] == F32(0.5)).all() and (g[~inside] == F32(FAR)).all()
    if case == "empty-mesh":
        assert bool((got == FAR).all())
    # device tensors in, the Camera class, same bytes
    cam = render.Camera(intrinsic_of(K), kw.get("near", 0.1), kw.get("far", FAR))
    one = cam.render(ext[0], torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev()), pixel_offset=kw.get("pixel_offset", 0.0))
    assert one.shape == (K[1], K[0]) and torch.equal(one, got[0])


def test_one_view_at_the_camera_resolution():
    v, f = scene_mesh(0)
    stats = {}
    got, offs = render.render_depth_batch([(v, f)], intrinsic_of(emu.SIM_INTRINSIC), [emu.six_views(SIZE, 1, 6)], device=dev(), stats=stats)
    same_bytes(got, sim_reference()[:1], "480x640 one view")
    tiles = (640 // 16) * (480 // 16)
    print(f"{stats['tile_pairs']} (triangle, tile) pairs survive the culling of {len(f) * tiles}")
    assert tiles <= stats["tile_pairs"] < len(f) * tiles // 2           # every tile sees the plane; most see little else


def test_ragged_batch_equals_single_calls_and_repeats():
    K = emu.SMALL_INTRINSIC
    counts = (6, 1, 3, 0)
    meshes = [scene_mesh(4), remu.icosphere((0.15, 0.15, 0.1), 0.05, 1), scene_mesh(5), scene_mesh(6)]
    exts = [emu.six_views(SIZE, n, 6) if n else np.zeros((0, 4, 4)) for n in counts]
    depth, offs = render.render_depth_batch(meshes, intrinsic_of(K), exts, device=dev())
    again, _ = render.render_depth_batch(meshes, intrinsic_of(K), exts, device=dev())
    assert offs.tolist() == [0, 6, 7, 10, 10] and depth.shape == (10, K[1], K[0]) and torch.equal(depth, again)
    for b, (m, e) in enumerate(zip(meshes, exts)):
        one = render.render_depth(m[0], m[1], intrinsic_of(K), e, device=dev())
        assert torch.equal(one, depth[offs[b]:offs[b + 1]])
    same_bytes(depth[6:7], remu.render_views(*meshes[1], exts[1], K), "batch scene 1")
    same_bytes(depth[7:10], remu.render_views(*meshes[2], exts[2], K), "batch scene 2")
    # an empty mesh inside a batch, and no scene at all
    d2, o2 = render.render_depth_batch([EMPTY, meshes[1]], intrinsic_of(K), [exts[1], exts[1]], device=dev())
    assert bool((d2[0] == FAR).all()) and torch.equal(d2[1], depth[6])
    d0, o0 = render.render_depth_batch([], intrinsic_of(K), [], device=dev())
    assert d0.shape == (0, K[1], K[0]) and o0.tolist() == [0]


# ------------------------------------------------------------------------------------------------ closed loop
def test_acquire_tsdf_equals_the_fusion_of_the_restatements_images():
    v, f = scene_mesh(0)
    K = emu.SIM_INTRINSIC
    lower, upper = perception.CLOUD_LOWER, perception.CLOUD_UPPER
    vol, pc, timing = render.acquire_tsdf(v, f, 6, device=dev(), lower=lower, upper=upper)
    assert isinstance(vol, perception.TSDFVolume) and vol.resolution == 40 and vol.size == SIZE and timing > 0
    t, w, g = emu.fuse(sim_reference(), emu.six_views(SIZE), K[2:], SIZE, 40)
    tsdf, weight = vol.state()
    for got, want, what in ((weight[0], w, "weight"), (tsdf[0], t, "tsdf"), (vol.grid()[0], g, "grid")):
        got = got.cpu().numpy()
        diff = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        print(f"acquire_tsdf {what}: {diff} of {want.size} words differ")
        assert diff == 0
    assert int((g != 0).sum()) > 1000
    p = pc.cpu().numpy()
    assert pc.is_cuda and p.dtype == F32 and len(p) > 1000 and (p >= lower).all() and (p <= upper).all()
    full = render.acquire_tsdf(v, f, 6, device=dev())[1]
    assert len(full) > len(p)
    # n of N, and the side view
    part = render.acquire_tsdf(v, f, 2, N=6, device=dev())[0]
    same_bytes(part.grid()[0], emu.fuse(sim_reference()[:2], emu.six_views(SIZE, 2, 6), K[2:], SIZE, 40)[2], "2 of 6 views")
    side = render.acquire_tsdf(v, f, 1, sideview=True, device=dev())[0]
    assert bool(side.grid().any())


def _net(sd7):
    from giga_amd import networks
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    return net.to(dev()).eval()


def test_acquire_tsdfs_equals_single_calls_and_feeds_the_planner(sd7):
    from giga_amd.detection import VGNImplicit
    meshes = [scene_mesh(7), scene_mesh(8), remu.merge(scene_mesh(9), remu.icosphere((0.15, 0.15, 0.09), 0.04, 2))]
    grids = render.acquire_tsdfs(meshes, 6, device=dev())
    assert grids.is_cuda and grids.shape == (3, 40, 40, 40)
    for b, (v, f) in enumerate(meshes):
        assert torch.equal(render.acquire_tsdf(v, f, 6, device=dev())[0].grid()[0], grids[b])
    planner = VGNImplicit(None, "giga", net=_net(sd7), best=True, force_detection=True, qual_th=0.6, out_th=0.1)
    sel = planner.plan_batch(grids, voxel_size=SIZE / 40)
    assert len(sel) == 3
    host = planner.plan_batch(torch.from_numpy(grids.cpu().numpy()).to(dev()), voxel_size=SIZE / 40)
    for a, b in zip(sel, host):
        assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["position"], b["position"])


# ------------------------------------------------------------------------------------------------ raw scenes
def test_write_raw_scenes_feeds_construct_dataset(tmp_path):
    from giga_amd import dataset
    raw, out = tmp_path / "raw", tmp_path / "data"
    meshes = [scene_mesh(10), scene_mesh(11), scene_mesh(12)]
    ids = ["s_a", "s_b", "s_c"]
    assert render.write_raw_scenes(raw, ids, meshes, 2, N=6, batch=2, device=dev()) == ids
    with (raw / "setup.json").open() as fh:
        setup = json.load(fh)
    intr = perception.CameraIntrinsic.from_dict(setup["intrinsic"])
    assert setup["size"] == SIZE and (intr.width, intr.height, intr.fx, intr.fy, intr.cx, intr.cy) == emu.SIM_INTRINSIC
    depth, ext = [], []
    for sid, (v, f) in zip(ids, meshes):
        with np.load(raw / "scenes" / (sid + ".npz")) as d:
            assert sorted(d.files) == ["depth_imgs", "extrinsics"]
            assert d["depth_imgs"].dtype == F32 and d["depth_imgs"].shape == (2, 480, 640)
            assert d["extrinsics"].dtype == F32 and d["extrinsics"].shape == (2, 7)
            depth.append(d["depth_imgs"]); ext.append(d["extrinsics"])
        assert torch.equal(torch.from_numpy(depth[-1]).to(dev()), render.render_depth(v, f, intr, emu.six_views(SIZE, 2, 6), device=dev()))
        assert np.allclose(np.stack([perception.extrinsic_matrix(e) for e in ext[-1]]), emu.six_views(SIZE, 2, 6), atol=1e-6)
    assert perception.construct_dataset(raw, out, batch=2, device=dev()) == ids
    want = perception.create_tsdfs(SIZE, 40, depth, intr, ext, dev()).cpu().numpy()
    for b, sid in enumerate(ids):
        got = dataset.read_voxel_grid(out, sid)
        assert got.shape == (1, 40, 40, 40) and np.array_equal(got[0].view(np.uint32), want[b].view(np.uint32)) and got.any()


# ------------------------------------------------------------------------------------------------ occupancy labels
BOXES = [((0.05, 0.06, 0.05), (0.12, 0.14, 0.11)), ((0.17, 0.15, 0.05), (0.26, 0.22, 0.19))]


def _box_distance(p, lo, hi):
    """distance of the points to the surface of the box, and whether they are inside"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = np.linalg.norm(np.maximum(np.maximum(lo - p, p - hi), 0.0), axis=1)
    inn = np.minimum(p - lo, hi - p).min(axis=1)
    inside = inn > 0
    return np.where(inside, inn, out), inside


def test_sample_iou_points_on_two_boxes():
    from giga_amd.eval import check_mesh_contains
    meshes = [remu.box_mesh(lo, hi) for lo, hi in BOXES]
    bounds = render.mesh_bounds(meshes)
    assert np.allclose(bounds, [[0.05, 0.06, 0.05], [0.26, 0.22, 0.19]])
    n = 4096
    gen = torch.Generator(device=dev()).manual_seed(11)
    points, occ = render.sample_iou_points(meshes, bounds, n, generator=gen)
    assert points.is_cuda and points.shape == (n, 3) and points.dtype == torch.float32 and occ.shape == (n,) and occ.dtype == torch.bool
    p = points.cpu().numpy().astype(np.float64)
    assert (p >= bounds[0] - 0.02 - 1e-6).all() and (p <= bounds[1] + 0.02 + 1e-6).all()
    assert p.min(axis=0)[0] < bounds[0, 0] and p.max(axis=0)[0] > bounds[1, 0]                  # the padding is used
    single = check_mesh_contains(meshes[0], points) | check_mesh_contains(meshes[1], points)
    assert torch.equal(occ, single)
    want = np.zeros(n, bool)
    for m in meshes:                                                                            # the float32 corners the mesh holds
        d, inside = _box_distance(p, m[0].min(axis=0), m[0].max(axis=0))
        assert d.min() > 1e-6, "draw from another seed: a point lies within 1e-6 of a face"
        want |= inside
    assert 100 < want.sum() < n - 100 and np.array_equal(occ.cpu().numpy(), want)
    # the same generator state draws the same points; uniform sampling covers the padded workspace
    again, _ = render.sample_iou_points(meshes, bounds, n, generator=torch.Generator(device=dev()).manual_seed(11))
    assert torch.equal(again, points)
    u, uo = render.sample_iou_points(meshes, bounds, n, uniform=True, generator=gen)
    assert float(u.min()) >= -0.02 - 1e-6 and float(u.max()) <= SIZE + 0.02 + 1e-6 and float(u.max()) > SIZE
    assert torch.equal(uo, check_mesh_contains(meshes[0], u) | check_mesh_contains(meshes[1], u))


def test_save_occ_directory_loads_through_the_dataset(tmp_path):
    from giga_amd import dataset, synth
    root, raw0, raw = tmp_path / "data", tmp_path / "raw0", tmp_path / "raw"
    synth.write_training_set(str(root), str(raw0), n_scenes=2, grasps_per_scene=2, seed=4)
    raw.mkdir()
    for name in ("grasps.csv", "setup.json"):
        shutil.copy(raw0 / name, raw / name)
    ids = sorted(p.name for p in (raw0 / "occ").iterdir())
    meshes = [remu.box_mesh(lo, hi) for lo, hi in BOXES]
    for sid in ids:
        render.save_occ(raw, sid, meshes, 500, 2, generator=torch.Generator(device=dev()).manual_seed(5))
    ds = dataset.GraspOccDataset(str(root), str(raw), num_point_occ=64)
    assert len(ds) == 4 and sorted(p.name for p in ds.occ_paths(ids[0])) == ["0000.npz", "0001.npz"]
    x, _, _, occ_points, occ = ds.item(0)
    assert x.shape == (40, 40, 40) and occ_points.shape == (64, 3) and occ.shape == (64,)
    with np.load(raw / "occ" / ids[0] / "0001.npz") as d:
        assert d["points"].dtype == np.float16 and d["points"].shape == (500, 3) and d["occ"].dtype == bool and 0 < d["occ"].sum() < 500
