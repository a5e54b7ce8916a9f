"""CPU tests of the depth renderer's semantics (the numpy restatement of tests/render_emu.py against the analytic ray caster of
tests/tsdf_emu.py and against hand-computed pixels), of giga_depth_render's argument validation without a device and of the host
logic of giga_amd.render."""
import ctypes
import os

import numpy as np
import pytest

import render_emu as remu
import tsdf_emu as emu
from giga_amd import _capi, render

F32 = np.float32
SIZE = 0.3
PIXEL_CAM = (32, 16, 64.0, 64.0, 16.0, 8.0)          # watertightness camera: identity extrinsic, 32x16 image
FAR = 2.0


# ------------------------------------------------------------------------------- the restatement against the analytic renderer
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_matches_the_analytic_ray_caster_on_plane_and_boxes(seed):
    # plane and boxes only, with the coordinates a float32 mesh can hold: the analytic caster and the mesh then describe the SAME
    # scene.  (With the seeds' float64 corners the mesh differs from the analytic scene by the float32 rounding of its vertices,
    # 3e-8 relative, which a grazing box side turns into up to 2 ulps of depth for seeds 1 and 2.)
    scene = emu.make_scene(seed)
    scene = {"plane_z": float(F32(scene["plane_z"])), "spheres": [],
             "boxes": [(np.asarray(lo, F32).astype(np.float64), np.asarray(hi, F32).astype(np.float64)) for lo, hi in scene["boxes"]]}
    v, f = remu.scene_to_mesh(scene)
    K = emu.SMALL_INTRINSIC
    ext = emu.six_views(SIZE)
    stats = {}
    got = remu.render_views(v, f, ext, K, 0.1, FAR, 0.0, stats)
    want = emu.render_views(scene, ext, K)
    print(f"seed {seed}: {len(f)} triangles, {stats['knife_edge']} knife-edge pixels, {stats['hits']} accepted pairs")
    assert stats["knife_edge"] == 0                                 # a condition on the input, not on the renderer
    assert got.shape == want.shape == (6, K[1], K[0]) and got.dtype == F32
    assert np.array_equal(got == F32(FAR), want == 0)               # hit / miss on every pixel
    assert (want > 0).all()                                         # (the plane fills these views)
    # both compute the same real number in double and round once
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print(f"max |restatement - analytic| = {err.max():.3e}, in ulps {np.max(err / np.spacing(want)):.2f}")
    assert (err <= np.spacing(want)).all()


# ------------------------------------------------------------------------------- watertightness
def watertight_square(flip):
    # cells of 2 pixels: at z = 0.5 one pixel is 1 / 128; the square covers columns 4 .. 28 and rows 2 .. 14, so pixel centres
    # fall on vertices, on axis-parallel edges and on the midpoints of diagonals.  Every coordinate is exact in float32.
    return remu.grid_square((4 - 16) / 128.0, (2 - 8) / 128.0, 2 / 128.0, 12, 6, 0.5, flip)


@pytest.mark.parametrize("flip", [False, True])
def test_no_cracks_on_shared_edges_and_vertices(flip):
    v, f = watertight_square(flip)
    assert np.array_equal(v.astype(np.float64), np.asarray(v, np.float64)) and len(f) == 144
    img = remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR)
    inside = np.zeros((16, 32), bool)
    inside[2:15, 4:29] = True
    assert (img[inside] == F32(0.5)).all()                          # exactly 0.5, no pixel of the outline's inside at far
    assert (img[~inside] == F32(FAR)).all()


# ------------------------------------------------------------------------------- near, far, behind the camera, pixel offset
def test_near_and_far_clipping():
    v, f = remu.box_mesh((-0.05, -0.05, 0.05), (0.05, 0.05, 0.3))    # straddles near = 0.1: the front face is rejected
    img = remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR)
    assert img[8, 16] == F32(0.3)                                   # the central ray meets front (0.05) and back (0.3) only
    assert abs(float(img[8, 0]) - 0.2) < 1e-7                       # d.x = -1/4 meets the side x = -0.05 at z = 0.2
    v, f = remu.box_mesh((-0.5, -0.5, 2.5), (0.5, 0.5, 3.0))        # beyond far
    assert (remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR) == F32(FAR)).all()
    v, f = remu.plane_mesh(0.5, 5.0)                                # 0.5 is exact: near = 0.5 and far = 0.5 both accept it
    assert (remu.render(v, f, np.eye(4), PIXEL_CAM, 0.5, FAR) == F32(0.5)).all()
    assert (remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, 0.5) == F32(0.5)).all()
    assert (remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, 0.25) == F32(0.25)).all()                 # behind far: float(far)


BEHIND = (np.array([[-1, 0.0625, 2], [1, 0.0625, 2], [0, 0.0625, -1]], F32), np.array([[0, 1, 2]], np.int32))


def test_triangle_with_a_vertex_behind_the_camera_covers_its_visible_pixels():
    # the triangle lies in the plane y = 1/16 below the optical axis, its third vertex behind the camera.  The ray of row v has
    # d.y = (v - 8) / 64 and meets the plane at z = (1/16) / d.y = 4 / (v - 8); at that depth the triangle is (z + 1) / 3 wide
    # to each side, more than the image (|d.x| <= 1/4).  By hand: pixel (12, 16) sees z = 1.
    v, f = BEHIND
    img = remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR)
    assert img[12, 16] == F32(1.0)
    for row in range(11, 16):
        assert np.allclose(img[row], 4.0 / (row - 8), rtol=1e-6, atol=0)
    assert (img[:10] == F32(FAR)).all()                             # rows above the axis meet the plane behind the camera; row 9 at z = 4


def test_pixel_offset_shifts_the_outline():
    # a square x, y in [-4/128, 4/128] at z = 0.5: image coordinates 12 .. 20 in x, 4 .. 12 in y
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    a = remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR, 0.0) != F32(FAR)
    b = remu.render(v, f, np.eye(4), PIXEL_CAM, 0.1, FAR, 0.5) != F32(FAR)
    want_a, want_b = np.zeros((16, 32), bool), np.zeros((16, 32), bool)
    want_a[4:13, 12:21] = True                                      # u in 12 .. 20
    want_b[4:12, 12:20] = True                                      # u + 0.5 in [12, 20]: u in 12 .. 19
    assert np.array_equal(a, want_a) and np.array_equal(b, want_b)


def test_skipped_triangles_and_the_empty_mesh():
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    base = remu.render(v, f, np.eye(4), PIXEL_CAM)
    bad_v = np.concatenate([v, [[np.nan, 0, 0.4], [0.1, 0.1, 0.4], [-0.1, 0.1, 0.4]]]).astype(F32)
    bad_f = np.concatenate([f, [[4, 5, 6]], [[0, 1, 7]], [[0, -1, 2]]]).astype(np.int32)      # a NaN vertex, two indices outside the mesh
    assert np.array_equal(remu.render(bad_v, bad_f, np.eye(4), PIXEL_CAM), base)
    empty = remu.render(np.zeros((0, 3), F32), np.zeros((0, 3), np.int32), np.eye(4), PIXEL_CAM)
    assert empty.shape == (16, 32) and (empty == F32(FAR)).all()


def test_shared_edge_is_decided_consistently():
    rng = np.random.default_rng(5)
    P, Q = rng.normal(size=3), rng.normal(size=3)
    for d in rng.normal(size=(100, 2)):
        n, m = remu.cross(P, Q), remu.cross(Q, P)
        assert (d[0] * n[0] + d[1] * n[1]) + n[2] == -((d[0] * m[0] + d[1] * m[1]) + m[2])


# ------------------------------------------------------------------------------- ABI validation without a device
_BUF = (ctypes.c_double * 256)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 30
IDENT = tuple(np.eye(4).reshape(-1))
OMIT = object()


def _arr(values, ctype):
    return NUL if values is None else (ctype * len(values))(*values)


def _render(vertices=A, voffs=(0, 8), triangles=A, toffs=(0, 12), view_offs=(0, 2), ext=IDENT * 2, cam=(500.0, 500.0, 32.0, 24.0) * 2,
            B=1, W=64, H=48, near=0.1, far=2.0, po=0.0, depth=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_depth_render(vertices, _arr(voffs, ctypes.c_int32), triangles, _arr(toffs, ctypes.c_int32),
                                         _arr(view_offs, ctypes.c_int32), _arr(ext, ctypes.c_double), _arr(cam, ctypes.c_double), B, W, H,
                                         near, far, po, depth, ws, ws_bytes, NUL)


def _with(seq, i, value):
    seq = list(seq)
    seq[i] = value
    return tuple(seq)


CAM2 = (500.0, 500.0, 32.0, 24.0) * 2


@pytest.mark.parametrize("kwargs, code", [
    (dict(B=-1), -1), (dict(B=_capi.MAX_SCENES + 1), -7),
    (dict(W=0), -1), (dict(H=0), -1), (dict(W=4097), -1), (dict(H=4097), -1), (dict(H=-3), -1),
    (dict(near=0.0), -1), (dict(near=-0.1), -1), (dict(near=float("nan")), -1), (dict(far=0.1), -1), (dict(far=0.05), -1),
    (dict(far=float("nan")), -1), (dict(far=float("inf")), -1), (dict(po=float("nan")), -1),
    (dict(voffs=None), -1), (dict(toffs=None), -1), (dict(view_offs=None), -1),
    (dict(voffs=(1, 8)), -1), (dict(toffs=(2, 12)), -1), (dict(view_offs=(1, 2)), -1),
    (dict(voffs=(0, -8)), -1), (dict(toffs=(0, -1)), -1), (dict(view_offs=(0, -2)), -1),
    (dict(B=2, voffs=(0, 8, 4), toffs=(0, 12, 12), view_offs=(0, 1, 2)), -1),
    (dict(B=2, voffs=(0, 8, 8), toffs=(0, 12, 6), view_offs=(0, 1, 2)), -1),
    (dict(B=2, voffs=(0, 8, 8), toffs=(0, 12, 12), view_offs=(0, 2, 1)), -1),
    (dict(W=4096, H=4096, view_offs=(0, 128), ext=IDENT * 128, cam=CAM2 * 64), -1),              # n W H = 2^31
    (dict(vertices=NUL), -1), (dict(triangles=NUL), -1), (dict(ext=None), -1), (dict(cam=None), -1), (dict(ws=NUL), -1),
    (dict(cam=_with(CAM2, 0, 0.0)), -1), (dict(cam=_with(CAM2, 5, 0.0)), -1), (dict(cam=_with(CAM2, 2, float("nan"))), -1),
    (dict(cam=_with(CAM2, 7, float("inf"))), -1), (dict(ext=_with(IDENT * 2, 3, float("nan"))), -1),
    (dict(ext=_with(IDENT * 2, 31, float("-inf"))), -1),
    (dict(depth=NUL), -6), (dict(ws_bytes=100), -4),
    (dict(B=0), 0), (dict(B=0, voffs=None, toffs=None, view_offs=None, ext=None, cam=None, vertices=NUL, triangles=NUL, depth=NUL), 0),
    (dict(view_offs=(0, 0), ext=None, cam=None, depth=NUL, ws=NUL), 0),                            # no views: nothing to do
])
def test_depth_render_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _render(**kwargs) == code


def test_depth_render_is_exported_and_declared():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_depth_render", "giga_depth_render_workspace_bytes"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    assert _capi.RENDER_MAX_IMAGE == int(hdr.split("#define GIGA_RENDER_MAX_IMAGE")[1].split()[0])
    assert L.giga_depth_render_workspace_bytes(0, 6, 8, 12) == 0 and L.giga_depth_render_workspace_bytes(1, -1, 8, 12) == 0
    assert L.giga_depth_render_workspace_bytes(_capi.MAX_SCENES + 1, 6, 8, 12) == 0
    assert L.giga_depth_render_workspace_bytes(4, 24, 100, 200) >= 8 + 3 * 5 * 4 + 24 * 4 + 24 * 20 * 8


# ------------------------------------------------------------------------------- host logic
def test_scene_mesh_scales_poses_and_rebases():
    v0, f0 = remu.box_mesh((0, 0, 0), (1, 2, 3))
    v1, f1 = remu.plane_mesh(0.0, 1.0)
    pose = np.eye(4)
    pose[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]               # quarter turn about z
    pose[:3, 3] = [0.5, 0.25, -1.0]
    v, f = render.scene_mesh([(v0, f0, 0.5, pose), (v1, f1, 2.0, np.eye(4))])
    assert v.dtype == F32 and f.dtype == np.int32 and v.shape == (12, 3) and f.shape == (14, 3)
    want = (v0.astype(np.float64) * 0.5) @ pose[:3, :3].T + pose[:3, 3]
    assert np.array_equal(v[:8], want.astype(F32)) and np.array_equal(v[8:], (v1.astype(np.float64) * 2.0).astype(F32))
    assert np.array_equal(v[7], np.array([0.5 - 1.0, 0.25 + 0.5, -1.0 + 1.5], F32))                # (1, 2, 3) / 2 turned and moved
    assert np.array_equal(f[:12], f0) and np.array_equal(f[12:], f1 + 8)
    v, f = render.scene_mesh([])
    assert v.shape == (0, 3) and f.shape == (0, 3) and v.dtype == F32 and f.dtype == np.int32


def test_acquire_extrinsics_are_the_reference_circle():
    for n, N in ((6, None), (3, 6), (1, None)):
        assert np.array_equal(render.acquire_extrinsics(n, N, SIZE), emu.six_views(SIZE, n, N))
    side = render.acquire_extrinsics(1, None, SIZE, sideview=True)
    assert side.shape == (1, 4, 4)
    eye = -side[0, :3, :3].T @ side[0, :3, 3]                        # camera centre: r = 2 size from (size/2, size/2, size/3)
    want = np.r_[SIZE / 2, SIZE / 2, SIZE / 3] + 2 * SIZE * np.r_[0.0, -np.sin(np.pi / 3), np.cos(np.pi / 3)]
    assert np.allclose(eye, want, atol=1e-12)
    assert render.SIM_INTRINSIC == emu.SIM_INTRINSIC and (render.SIM_NEAR, render.SIM_FAR) == (0.1, 2.0)
    assert np.allclose(render.pose_list(side[0])[4:], side[0, :3, 3])


def test_save_occ_file_names_dtypes_and_shapes(tmp_path, monkeypatch):
    import torch
    seen = {}

    def fake(mesh_list, bounds, num_point, padding=0.02, uniform=False, size=0.3, generator=None, device=None):
        seen.update(bounds=bounds, n=num_point, uniform=uniform)
        g = torch.Generator().manual_seed(3)
        p = torch.rand((num_point, 3), generator=g)
        return p, p[:, 0] > 0.5
    monkeypatch.setattr(render, "sample_iou_points", fake)
    meshes = [remu.box_mesh((0.1, 0.1, 0.05), (0.15, 0.2, 0.1)), remu.box_mesh((0.2, 0.05, 0.05), (0.25, 0.1, 0.2))]
    root = render.save_occ(tmp_path, "abc", meshes, 50, 3, uniform=True)
    assert seen["n"] == 150 and seen["uniform"] is True
    assert np.allclose(seen["bounds"], [[0.1, 0.05, 0.05], [0.25, 0.2, 0.2]])
    assert sorted(os.listdir(root)) == ["0000.npz", "0001.npz", "0002.npz"] and root == str(tmp_path / "occ" / "abc")
    p = torch.rand((150, 3), generator=torch.Generator().manual_seed(3)).numpy()
    for i in range(3):
        with np.load(os.path.join(root, "%04d.npz" % i)) as d:
            assert sorted(d.files) == ["occ", "points"]
            assert d["points"].dtype == np.float16 and d["points"].shape == (50, 3) and d["occ"].dtype == bool and d["occ"].shape == (50,)
            assert np.array_equal(d["points"], p[50 * i:50 * (i + 1)].astype(np.float16))
            assert np.array_equal(d["occ"], p[50 * i:50 * (i + 1), 0] > 0.5)
    with pytest.raises(FileExistsError):
        render.save_occ(tmp_path, "abc", meshes, 50, 3)


def test_rendering_needs_a_device():
    import torch
    v, f = remu.plane_mesh(0.5, 0.1)
    with pytest.raises(_capi.GigaHipError):
        render.render_depth(torch.from_numpy(v), torch.from_numpy(f), render.sim_intrinsic(), [np.eye(4)], device="cpu")
    with pytest.raises(_capi.GigaHipError):
        render.sample_iou_points([(v, f)], np.zeros((2, 3)), 10, device="cpu")
    import giga_amd
    assert giga_amd.render_depth is render.render_depth and giga_amd.save_occ is render.save_occ
