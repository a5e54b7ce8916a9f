"""CPU tests of the depth fusion: closed forms pin the numpy restatement (tests/tsdf_emu.py) that the GPU tests compare bytes
with, the C ABI rejects bad arguments without a device, and the host-side Python of giga_amd.perception behaves."""
import ctypes
import json

import numpy as np
import pytest

import tsdf_emu as emu
from giga_amd import _capi, perception

F32 = np.float32
SIZE, R = 0.3, 40
VOXEL = SIZE / R
TRUNC = 4 * VOXEL


def down_camera(x, y, z):
    """Extrinsic of a camera at (x, y, z) that looks along -z of the task frame (image x = task x, image y = -task y)."""
    E = np.diag([1.0, -1.0, -1.0, 1.0])
    E[:3, 3] = [-x, y, z]
    return E


PLANE_CAM = down_camera(0.15, 0.15, 0.6)
PLANE_K = (200.0, 190.0, 31.5, 23.5)
PLANE_W, PLANE_H = 64, 48


def plane_closed_form(D):
    """Per voxel, one view of a fronto-parallel plane at depth D, written from the geometry in float64: (touched, tsdf, safe);
    `safe` leaves out the voxels within 1e-3 pixel of the image border or 1e-7 m of the truncation, where float64 and the
    restatement's stated precisions may fall on different sides."""
    c = (np.arange(R) + 0.5) * VOXEL
    X, Y, Z = np.meshgrid(c, c, c, indexing="ij")
    fx, fy, cx, cy = PLANE_K
    zc = 0.6 - Z
    uf, vf = (X - 0.15) * fx / zc + cx + 0.5, -(Y - 0.15) * fy / zc + cy + 0.5
    u, v = np.floor(uf), np.floor(vf)
    seen = (u >= 0) & (u < PLANE_W) & (v >= 0) & (v < PLANE_H)
    m = np.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1)
    sdf = (D - zc) * m
    safe = (np.abs(sdf + TRUNC) > 1e-7)
    for f, n in ((uf, PLANE_W), (vf, PLANE_H)):
        safe &= (np.abs(f) > 1e-3) & (np.abs(f - n) > 1e-3)
    return seen & (sdf > -TRUNC), np.clip(sdf / TRUNC, None, 1.0), safe


def test_fronto_parallel_plane_matches_the_closed_form():
    D = 0.6 - 0.1234                                        # the plane z = 0.1234 of the task frame
    depth = np.full((1, PLANE_H, PLANE_W), D, F32)
    t, w, g = emu.fuse(depth, [PLANE_CAM], PLANE_K, SIZE, R)
    touched, want, safe = plane_closed_form(float(F32(D)))
    assert touched.any() and not touched.all() and safe.mean() > 0.99
    assert np.array_equal((w != 0)[safe], touched[safe]) and np.all(w[w != 0] == 1)
    on = touched & safe
    assert np.abs(t[on] - want[on]).max() <= 2e-6            # float32 roundings of m, sdf, the product and the quotient
    assert np.all(t[~touched & safe] == 0)
    band = on & (want >= -0.98 + 1e-5) & (want < 0.98 - 1e-5)
    assert band.any() and np.abs(g[band] - (want[band] + 1) / 2).max() <= 2e-6
    out = safe & (~touched | (want < -0.98 - 1e-5) | (want >= 0.98 + 1e-5))
    assert out.any() and np.all(g[out] == 0)
    # above the plane the distance is positive, below it negative, and beyond the truncation nothing is written
    z = (np.arange(R) + 0.5) * VOXEL
    col, wcol = t[20, 20], w[20, 20]
    assert np.all(col[z > 0.1234 + 1e-3] > 0) and np.all(col[(z < 0.1234 - 1e-3) & (wcol != 0)] < 0)
    assert np.all(wcol[z < 0.1234 - TRUNC * 1.01] == 0) and np.all(wcol[z > 0.1234] == 1)


def test_voxels_behind_outside_or_beyond_the_range_are_untouched():
    depth = np.full((1, PLANE_H, PLANE_W), 0.5, F32)
    # camera below the volume looking down: every voxel is behind it
    t, w, _ = emu.fuse(depth, [down_camera(0.15, 0.15, -0.1)], PLANE_K, SIZE, R)
    assert not w.any() and not t.any()
    # camera far to the side: every voxel projects outside the image
    t, w, _ = emu.fuse(depth, [down_camera(5.0, 0.15, 0.6)], PLANE_K, SIZE, R)
    assert not w.any()
    # depth at or beyond depth_trunc = 2 counts as no measurement; so do 0, negative and NaN pixels
    for value in (2.0, 3.5, 0.0, -1.0, np.nan):
        t, w, _ = emu.fuse(np.full((1, PLANE_H, PLANE_W), value, F32), [PLANE_CAM], PLANE_K, SIZE, R)
        assert not w.any() and not t.any(), value
    # part of the image empty: exactly the voxels that project there stay untouched
    depth = np.full((1, PLANE_H, PLANE_W), 0.45, F32)
    depth[0, :, :32] = 0
    t, w, _ = emu.fuse(depth, [PLANE_CAM], PLANE_K, SIZE, R)
    x = (np.arange(R) + 0.5) * VOXEL
    u = np.floor((x[:, None] - 0.15) * PLANE_K[0] / (0.6 - x[None, :]) + PLANE_K[2] + 0.5)      # (x, z)
    assert w.any() and not w[(u < 32)[:, None, :] & np.ones((R, R, R), bool)].any()


def test_identical_views_repeat_and_different_views_average():
    d1 = np.full((1, PLANE_H, PLANE_W), 0.45, F32)
    d2 = np.full((1, PLANE_H, PLANE_W), 0.47, F32)
    t1, w1, g1 = emu.fuse(d1, [PLANE_CAM], PLANE_K, SIZE, R)
    t2, w2, _ = emu.fuse(d2, [PLANE_CAM], PLANE_K, SIZE, R)
    tt, ww, gg = emu.fuse(np.concatenate((d1, d1)), [PLANE_CAM, PLANE_CAM], PLANE_K, SIZE, R)
    assert np.array_equal(ww, 2 * w1) and np.abs(tt - t1).max() <= 1e-7 and np.abs(gg - g1).max() <= 1e-7
    ta, wa, _ = emu.fuse(np.concatenate((d1, d2)), [PLANE_CAM, PLANE_CAM], PLANE_K, SIZE, R)
    assert np.array_equal(wa, w1 + w2)
    both = (w1 == 1) & (w2 == 1)
    assert both.any() and np.abs(ta[both] - (t1[both].astype(np.float64) + t2[both]) / 2).max() <= 1e-7
    only1 = (w1 == 1) & (w2 == 0)
    assert np.array_equal(ta[only1], t1[only1])
    # a second call continues the running average of the first
    t, w = np.zeros((R, R, R), F32), np.zeros((R, R, R), F32)
    emu.integrate(t, w, d1, [PLANE_CAM], PLANE_K, SIZE)
    emu.integrate(t, w, d2, [PLANE_CAM], PLANE_K, SIZE)
    assert np.array_equal(t, ta) and np.array_equal(w, wa)


def test_cloud_points_of_the_plane_lie_on_the_plane():
    """A camera 1.95 m above a voxel centre sees the 5 x 5 columns around it nearly along its axis.  The two ends of a z-edge
    have m factors that differ by at most (r / z_c)^2 (voxel / z_c) = 6e-7 (r = 0.021 m, z_c = 1.8 m), which moves the
    interpolated crossing by a quarter of that in voxels; the float32 roundings of m, sdf and tsdf move it by 2e-7 voxels, and
    storing z < 0.125 as float32 by 3.7e-9 m = 5e-7 voxels: together below the bound of 1e-6 voxels."""
    K = (6000.0, 6000.0, 50.0, 50.0)
    cam = down_camera(20.5 * VOXEL, 20.5 * VOXEL, 1.95)
    for plane_z in (0.1234, 0.0791, 0.1100):
        d = F32(1.95 - plane_z)
        t, w = np.zeros((R, R, R), F32), np.zeros((R, R, R), F32)
        emu.integrate(t, w, np.full((1, 101, 101), d), [cam], K, SIZE)
        pts = emu.cloud(t, w, SIZE)
        assert pts.shape == (25, 3) and pts.dtype == F32
        assert np.abs(pts[:, 2].astype(np.float64) - (1.95 - float(d))).max() <= VOXEL * 1e-6
        # only z-edges cross a horizontal plane; x and y are voxel centres, in cell order
        centres = ((np.arange(18, 23) + 0.5) * VOXEL).astype(F32)
        assert np.array_equal(pts[:, 0], np.repeat(centres, 5)) and np.array_equal(pts[:, 1], np.tile(centres, 5))


def test_cloud_restatement_on_a_hand_made_volume():
    R5 = 6
    t, w = np.zeros((R5,) * 3, F32), np.zeros((R5,) * 3, F32)
    t[1, 2, 3], t[2, 2, 3], t[1, 3, 3], t[1, 2, 4] = 0.5, -0.25, -0.5, 0.99
    w[1, 2, 3] = w[2, 2, 3] = w[1, 3, 3] = w[1, 2, 4] = 1
    t[4, 1, 1], t[5, 1, 1], w[4, 1, 1], w[5, 1, 1] = 0.3, -0.3, 1, 1           # neighbour index 5 is not < R - 1: no point
    t[0, 0, 0], t[0, 0, 1], w[0, 0, 0] = 0.3, -0.3, 1                           # neighbour never observed: no point
    pts = emu.cloud(t, w, 0.6)
    vl = 0.1
    p0 = (np.array([1, 2, 3]) + 0.5) * vl
    want = np.array([[(p0[0] * 0.25 + (p0[0] + vl) * 0.5) / 0.75, p0[1], p0[2]],
                     [p0[0], (p0[1] * 0.5 + (p0[1] + vl) * 0.5) / 1.0, p0[2]]])    # z neighbour 0.99 is outside the band
    assert pts.shape == (2, 3) and np.abs(pts - want).max() <= 1e-7


def test_test_scenes_have_few_knife_edge_voxel_views():
    """The GPU tests compare bytes; should an operation of the device ever turn out not to be correctly rounded, only knife-edge
    voxel-views could differ.  Their number in the test scenes stays far below 0.1 % per scene."""
    K = emu.SMALL_INTRINSIC
    for seed in (1, 2, 3):
        ext = emu.six_views(SIZE)
        depth = emu.render_views(emu.make_scene(seed), ext, K)
        assert (depth > 0).mean() > 0.5
        stats = {}
        t, w, g = emu.fuse(depth, ext, K[2:], SIZE, R, stats=stats)
        assert stats["voxel_views"] == 6 * R ** 3 and stats["knife_edge"] <= 1e-3 * stats["voxel_views"], stats
        assert (g > 0).sum() > 2000 and len(emu.cloud(t, w, SIZE)) > 500


# ------------------------------------------------------------------------------------------------------- C ABI
_BUF = (ctypes.c_double * 256)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 30
IDENT = tuple(np.eye(4).reshape(-1))


def _arr(values, ctype):
    return (ctype * len(values))(*values)


def _integrate(depth=A, offs=(0, 2), ext=IDENT * 2, cam=(500.0, 500.0, 32.0, 24.0) * 2, B=1, W=64, H=48, length=0.3, R=40, trunc=0.03,
               scale=1.0, dtrunc=2.0, tsdf=A, weight=A, grid=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_tsdf_integrate(depth, _arr(offs, ctypes.c_int32) if offs is not None else NUL,
                                           _arr(ext, ctypes.c_double) if ext is not None else NUL,
                                           _arr(cam, ctypes.c_double) if cam is not None else NUL, B, W, H, length, R, trunc, scale, dtrunc,
                                           tsdf, weight, grid, ws, ws_bytes, NUL)


def _count(tsdf=A, weight=A, B=1, R=40, ws=A, ws_bytes=BIG, counts=A):
    return _capi.lib().giga_tsdf_cloud_count(tsdf, weight, B, R, ws, ws_bytes, counts, NUL)


def _emit(tsdf=A, weight=A, B=1, R=40, length=0.3, ws=A, ws_bytes=BIG, points=A, cap=16, shortfall=A):
    return _capi.lib().giga_tsdf_cloud_emit(tsdf, weight, B, R, length, ws, ws_bytes, points, cap, shortfall, NUL)


def test_fusion_entries_are_exported_and_declared():
    import os
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_tsdf_integrate", "giga_tsdf_integrate_workspace_bytes", "giga_tsdf_cloud_workspace_bytes",
                 "giga_tsdf_cloud_count", "giga_tsdf_cloud_emit"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    assert _capi.TSDF_MAX_R == int(hdr.split("#define GIGA_TSDF_MAX_R")[1].split()[0])


def _bad_cam(i, value):
    cam = [500.0, 500.0, 32.0, 24.0] * 2
    cam[i] = value
    return tuple(cam)


def _bad_ext(i, value):
    ext = list(IDENT * 2)
    ext[i] = value
    return tuple(ext)


BIG_B = dict(B=_capi.MAX_SCENES + 1)


@pytest.mark.parametrize("call, kwargs, code", [
    (_integrate, dict(B=-1), -1), (_integrate, BIG_B, -7), (_integrate, dict(R=1), -1), (_integrate, dict(R=0), -1),
    (_integrate, dict(R=513), -1), (_integrate, dict(W=0), -1), (_integrate, dict(H=0), -1), (_integrate, dict(W=1 << 20), -1),
    (_integrate, dict(H=-3), -1), (_integrate, dict(length=0.0), -1), (_integrate, dict(length=float("nan")), -1),
    (_integrate, dict(length=float("inf")), -1), (_integrate, dict(trunc=0.0), -1), (_integrate, dict(trunc=float("nan")), -1),
    (_integrate, dict(scale=0.0), -1), (_integrate, dict(dtrunc=float("nan")), -1),
    (_integrate, dict(offs=None), -1), (_integrate, dict(offs=(1, 2)), -1), (_integrate, dict(offs=(0, -2)), -1),
    (_integrate, dict(B=2, offs=(0, 2, 1)), -1),
    (_integrate, dict(cam=_bad_cam(0, 0.0)), -1), (_integrate, dict(cam=_bad_cam(5, 0.0)), -1),
    (_integrate, dict(cam=_bad_cam(2, float("nan"))), -1), (_integrate, dict(cam=_bad_cam(7, float("inf"))), -1),
    (_integrate, dict(ext=_bad_ext(3, float("nan"))), -1), (_integrate, dict(ext=_bad_ext(31, float("-inf"))), -1),
    (_integrate, dict(ext=None), -1), (_integrate, dict(cam=None), -1), (_integrate, dict(depth=NUL), -1),
    (_integrate, dict(tsdf=NUL), -1), (_integrate, dict(weight=NUL), -1), (_integrate, dict(ws=NUL), -1),
    (_integrate, dict(ws_bytes=100), -4), (_integrate, dict(B=0), 0), (_integrate, dict(B=0, offs=None, ext=None, cam=None, depth=NUL), 0),
    (_count, dict(tsdf=NUL), -1), (_count, dict(weight=NUL), -1), (_count, dict(ws=NUL), -1), (_count, dict(counts=NUL), -1),
    (_count, dict(B=-1), -1), (_count, BIG_B, -7), (_count, dict(R=1), -1), (_count, dict(R=600), -1), (_count, dict(ws_bytes=100), -4),
    (_count, dict(B=0), 0),
    (_emit, dict(tsdf=NUL), -1), (_emit, dict(weight=NUL), -1), (_emit, dict(ws=NUL), -1), (_emit, dict(points=NUL), -6),
    (_emit, dict(B=-1), -1), (_emit, BIG_B, -7), (_emit, dict(R=1), -1), (_emit, dict(length=0.0), -1),
    (_emit, dict(length=float("nan")), -1), (_emit, dict(ws_bytes=100), -4), (_emit, dict(B=0), 0),
])
def test_fusion_entries_reject_invalid_arguments_without_a_device(call, kwargs, code):
    assert call(**kwargs) == code


def test_fusion_workspace_sizes():
    L = _capi.lib()
    assert L.giga_tsdf_integrate_workspace_bytes(0, 6) == 0 and L.giga_tsdf_integrate_workspace_bytes(1, -1) == 0
    assert L.giga_tsdf_integrate_workspace_bytes(_capi.MAX_SCENES + 1, 6) == 0
    assert L.giga_tsdf_integrate_workspace_bytes(4, 24) >= 5 * 4 + 24 * 20 * 8
    assert L.giga_tsdf_cloud_workspace_bytes(0, 40) == 0 and L.giga_tsdf_cloud_workspace_bytes(1, 1) == 0
    assert L.giga_tsdf_cloud_workspace_bytes(2, 40) >= 2 * (40 ** 3 // 256) * 4 + 3 * 8


# ------------------------------------------------------------------------------------------------------- Python host logic
def test_camera_intrinsic_round_trip():
    K = perception.CameraIntrinsic(640, 480, 540.0, 541.0, 320.0, 240.5)
    assert (K.width, K.height, K.fx, K.fy, K.cx, K.cy) == (640, 480, 540.0, 541.0, 320.0, 240.5)
    data = K.to_dict()
    assert data == {"width": 640, "height": 480, "K": [540.0, 0.0, 320.0, 0.0, 541.0, 240.5, 0.0, 0.0, 1.0]}
    back = perception.CameraIntrinsic.from_dict(json.loads(json.dumps(data)))
    assert np.array_equal(back.K, K.K) and (back.width, back.height) == (640, 480)


def test_the_three_extrinsic_forms_give_the_same_matrix():
    rng = np.random.default_rng(5)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    pose = np.r_[q, rng.normal(size=3)]
    want = emu.quat_matrix(pose)
    assert np.abs(want[:3, :3] @ want[:3, :3].T - np.eye(3)).max() <= 1e-15

    class T:
        def as_matrix(self):
            return want.copy()
    for form in (pose, list(pose), want, want.tolist(), T()):
        got = perception.extrinsic_matrix(form)
        assert got.shape == (4, 4) and got.dtype == np.float64 and np.abs(got - want).max() <= 1e-15
    for bad in (np.zeros(6), np.zeros((3, 4)), [1.0, 2.0]):
        with pytest.raises(ValueError):
            perception.extrinsic_matrix(bad)


def test_restatement_on_a_pose_list_equals_the_matrix():
    ext = emu.six_views(SIZE)
    from scipy.spatial.transform import Rotation
    poses = [np.r_[Rotation.from_matrix(E[:3, :3]).as_quat(), E[:3, 3]] for E in ext]
    mats = np.stack([perception.extrinsic_matrix(p) for p in poses])
    K = emu.SMALL_INTRINSIC
    depth = emu.render_views(emu.make_scene(4), mats, K)
    a = emu.fuse(depth, mats, K[2:], SIZE, R)
    b = emu.fuse(depth, np.stack([emu.quat_matrix(p) for p in poses]), K[2:], SIZE, R)
    # the two quaternion-to-matrix routes agree to an ulp or two of the matrix entries: a voxel-view on a knife edge may fall
    # on the other side, everything else agrees to float32 rounding
    assert np.abs(mats - np.stack([emu.quat_matrix(p) for p in poses])).max() <= 1e-15
    same = a[1] == b[1]
    assert same.mean() >= 0.999 and np.abs(a[0][same] - b[0][same]).max() <= 1e-6


def test_camera_on_sphere_looks_at_the_origin():
    origin = np.eye(4)
    origin[:3, 3] = [0.15, 0.15, 0.0]
    for phi in (0.0, 1.0, 4.0):
        E = perception.camera_on_sphere(origin, 0.6, np.pi / 6, phi)
        assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() <= 1e-14 and np.linalg.det(E[:3, :3]) > 0
        assert np.abs(E @ np.r_[0.15, 0.15, 0.0, 1.0] - np.r_[0, 0, 0.6, 1]).max() <= 1e-14           # on the optical axis, 0.6 away
        eye = -E[:3, :3].T @ E[:3, 3]
        want = np.r_[0.15, 0.15, 0] + 0.6 * np.r_[np.sin(np.pi / 6) * np.cos(phi), np.sin(np.pi / 6) * np.sin(phi), np.cos(np.pi / 6)]
        assert np.abs(eye - want).max() <= 1e-14
        assert (E[:3, :3] @ np.r_[0, 0, 1.0])[1] < 0                  # task z points up in the image (image y runs down)
    # the origin may come in any extrinsic form
    assert np.allclose(perception.camera_on_sphere([0, 0, 0, 1, 0.15, 0.15, 0.0], 0.6, np.pi / 6, 1.0),
                       perception.camera_on_sphere(origin, 0.6, np.pi / 6, 1.0), atol=1e-15)


def _raw_dataset(root, n_scenes, views=3):
    K = perception.CameraIntrinsic(*emu.SMALL_INTRINSIC)
    (root / "scenes").mkdir(parents=True)
    with (root / "setup.json").open("w") as f:
        json.dump({"size": SIZE, "intrinsic": K.to_dict(), "max_opening_width": 0.08, "finger_depth": 0.05}, f)
    from scipy.spatial.transform import Rotation
    ids = []
    for s in range(n_scenes):
        ext = emu.six_views(SIZE, views, 6)
        depth = emu.render_views(emu.make_scene(100 + s), ext, emu.SMALL_INTRINSIC)
        poses = np.stack([np.r_[Rotation.from_matrix(E[:3, :3]).as_quat(), E[:3, 3]] for E in ext])
        ids.append(f"scene{s:02d}")
        np.savez_compressed(root / "scenes" / (ids[-1] + ".npz"), depth_imgs=depth, extrinsics=poses)
    (root / "scenes" / "notes.txt").write_text("not a scene")
    return ids


def test_construct_dataset_argument_handling(tmp_path, monkeypatch):
    raw = tmp_path / "raw"
    ids = _raw_dataset(raw, 5)
    calls = []

    def fake(size, resolution, depth_batches, intrinsic, extrinsics_batches, device=None):
        calls.append(([d.shape for d in depth_batches], [e.shape for e in extrinsics_batches], size, resolution, intrinsic.width))
        B = len(depth_batches)
        grids = np.arange(B, dtype=F32)[:, None, None, None] + np.zeros((B, resolution, resolution, resolution), F32)
        pc = np.array([[0.1, 0.1, 0.1], [0.01, 0.1, 0.1], [0.1, 0.1, 0.05], [0.25, 0.25, 0.25], [0.1, 0.29, 0.1]], F32)
        return grids, [pc] * B

    monkeypatch.setattr(perception, "_fuse_to_host", fake)
    with pytest.raises(NotImplementedError):
        perception.construct_dataset(raw, tmp_path / "noise", add_noise="dex")
    with pytest.raises(ValueError):
        perception.construct_dataset(raw, tmp_path / "zero", batch=0)
    assert not calls and not (tmp_path / "noise").exists()
    out = tmp_path / "data"
    done = perception.construct_dataset(raw, out, batch=2)
    assert done == ids and [len(c[0]) for c in calls] == [2, 2, 1]
    assert calls[0][0] == [(3, 37, 53)] * 2 and calls[0][1] == [(3, 7)] * 2 and calls[0][2:] == (SIZE, 40, 53)
    from giga_amd.dataset import read_voxel_grid
    for k, scene in enumerate(ids):
        g = read_voxel_grid(out, scene)
        assert g.shape == (1, 40, 40, 40) and g.dtype == F32 and np.all(g == k % 2)
        pc = np.load(out / "point_clouds" / (scene + ".npz"))["pc"]
        assert pc.shape == (2, 3) and np.allclose(pc, [[0.1, 0.1, 0.1], [0.25, 0.25, 0.25]]) and pc.dtype == np.float64
    with pytest.raises(FileExistsError):
        perception.construct_dataset(raw, out)
    calls.clear()
    perception.construct_dataset(raw, tmp_path / "single", single_view=True, batch=32)
    assert len(calls) == 1 and calls[0][0] == [(1, 37, 53)] * 5 and calls[0][1] == [(1, 7)] * 5


def test_fusion_needs_a_device():
    with pytest.raises(_capi.GigaHipError):
        perception.TSDFVolume(0.3, 40, device="cpu")
    with pytest.raises(_capi.GigaHipError):
        perception.create_tsdfs(0.3, 40, [], perception.CameraIntrinsic(*emu.SMALL_INTRINSIC), [], device="cpu")
