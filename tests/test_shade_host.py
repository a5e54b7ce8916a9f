"""CPU tests of the colour renderer's semantics (the two forms of tests/shade_emu.py against each other and against hand-computed
pixels), of the camera helpers and the PNG writer of giga_amd.visual, of the supersampling parameters, and of the validation of
giga_color_render / giga_image_downsample without a device."""
import ctypes
import math
import os
import struct
import zlib

import numpy as np
import pytest

import render_emu as remu
import shade_emu as semu
from giga_amd import _capi, perception, render, visual

F32 = np.float32
FAR = 2.0
PIXEL_CAM = semu.PIXEL_CAM
RED = np.array([[201, 90, 33, 255]], np.uint8)


# ------------------------------------------------------------------------------- the two forms of the restatement
@pytest.mark.parametrize("case", list(semu.CASES))
def test_vectorised_and_scalar_forms_agree_byte_for_byte(case):
    c = semu.CASES[case]()
    a, b = semu.render_case(c), semu.render_case(c, form=semu.render_scalar)
    for x, y, what in zip(a, b, ("colour", "depth", "index")):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), (case, what)
    assert a[0].dtype == np.uint8 and a[1].dtype == F32 and a[2].dtype == np.int32
    hit = a[2] >= 0
    assert (a[0][hit][:, 3] == 255).all() and (a[0][~hit] == np.asarray(c[4].get("background", semu.WHITE), np.uint8)).all()
    assert np.array_equal(a[1], remu.render_views(*c[0], c[3], c[2], c[4].get("near", 0.1), c[4].get("far", FAR), c[4].get("pixel_offset", 0.0)))


def test_forms_agree_on_the_full_size_view_and_the_supersampled_scenes():
    (v, f), colors, K, ext, kw = semu.FULL()
    a = semu.render(v, f, colors, ext[0], K)
    pixels = [(r, c) for r in range(0, K[1], 7) for c in range(0, K[0], 7)]          # every 7th row and column: 6 348 pixels
    b = semu.render_scalar(v, f, colors, ext[0], K, pixels=pixels)
    rows, cols = np.array(pixels).T
    for x, y in zip(a, b):
        assert np.array_equal(x[rows, cols], y[rows, cols])
    for k in (2, 3):
        (v, f), colors, K, ext, kw = semu.SUPER()
        Kf, po = semu.supersample_camera(K, 0.0, k)
        for x, y in zip(semu.render(v, f, colors, ext[0], Kf, pixel_offset=po), semu.render_scalar(v, f, colors, ext[0], Kf, pixel_offset=po)):
            assert np.array_equal(x, y)


def test_tile_icosphere_sits_in_one_tile():
    (v, f), colors, K, ext, kw = semu.CASES["tile-icosphere-1280"]()
    rgba, depth, index = semu.render(v, f, colors, ext[0], K)
    rows, cols = np.nonzero(index >= 0)
    assert len(f) == 1280 > 384 and len(rows) > 16
    assert rows.min() // 16 == rows.max() // 16 and cols.min() // 16 == cols.max() // 16
    # the whole projected sphere, not only the pixel centres it covers, lies inside that tile
    cam = remu.camera_vertices(v, ext[0])
    pu, pv = cam[:, 0] / cam[:, 2] * K[2] + K[4], cam[:, 1] / cam[:, 2] * K[3] + K[5]
    assert 16 < pu.min() and pu.max() < 31 and 0 < pv.min() and pv.max() < 15
    assert len(np.unique(rgba[index >= 0], axis=0)) > 8              # per-face colours show


# ------------------------------------------------------------------------------- hand-computed pixels
def test_facing_triangle_under_the_headlight_keeps_its_colour_on_the_axis():
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    for ambient in (0.0, 0.25, 0.3, 1.0):
        rgba, depth, index = semu.render(v, f, np.repeat(RED, 2, 0), np.eye(4), PIXEL_CAM, ambient=ambient)
        # pixel (8, 16) is the optical axis: d = (0, 0, 1), p = (0, 0, 1/2), n = (0, 0, +-2^-8), L = -p: |n.L| = sqrt(q), k = 1
        assert tuple(rgba[8, 16]) == (201, 90, 33, 255) and depth[8, 16] == F32(0.5) and index[8, 16] == 0
        assert tuple(rgba[0, 0]) == semu.WHITE and index[0, 0] == -1 and depth[0, 0] == F32(FAR)       # a miss: the background
    # off the axis the headlight's cosine falls: on a large plane pixel (8, 31) has d = (15/64, 0, 1), cos = 1 / |d| = 0.97359,
    # k = 1/4 + 3/4 cos = 0.98019: 197.02, 88.22, 32.35 (+ 0.5, floor)
    v, f = remu.plane_mesh(0.5, 1.0)
    rgba = semu.render(v, f, np.repeat(RED, 2, 0), np.eye(4), PIXEL_CAM, ambient=0.25)[0]
    assert tuple(rgba[8, 31]) == (197, 88, 32, 255) and tuple(rgba[8, 16]) == (201, 90, 33, 255)


def test_plane_tilted_sixty_degrees_to_a_directional_light():
    v, f = remu.plane_mesh(0.5, 1.0)
    light = (math.sqrt(3.0), 0.0, -1.0, 0.0)                         # 60 degrees off the plane's normal (0, 0, +-1), towards the camera side
    rgba, _, index = semu.render(v, f, np.repeat(RED, 2, 0), np.eye(4), PIXEL_CAM, light=light, ambient=0.25)
    # k = 1/4 + (3/4) / 2 = 0.625 on every pixel: 125.625, 56.25, 20.625 (+ 0.5, floor): no value near a rounding boundary
    assert (index >= 0).all() and (rgba == np.array([126, 56, 21, 255], np.uint8)).all()
    rgba = semu.render(v, f, np.repeat(RED, 2, 0), np.eye(4), PIXEL_CAM, light=(0.0, 0.0, 1.0, 0.0), ambient=0.25)[0]
    assert (rgba == RED[0]).all()                                    # along the normal, from behind: two-sided, k = 1


def test_q_zero_or_not_finite_leaves_the_ambient_term():
    # a zero-area triangle has S = d . ((b - a) x (c - a)) = 0 in exact arithmetic and is not hit; it could win only through
    # rounding, which exact coordinates cannot provoke.  The branch it would take (q = 0) is reached with L = 0 instead: a point
    # light on the surface point itself; q = inf with a light 1e200 away.
    v, f = remu.plane_mesh(0.5, 4 / 128.0)
    degenerate = np.array([[-0.03125, 0, 0.5], [0, 0, 0.5], [0.03125, 0, 0.5]], F32), np.array([[0, 1, 2]], np.int32)
    assert (semu.render(*degenerate, RED, np.eye(4), PIXEL_CAM)[2] == -1).all()
    for form in (semu.render, semu.render_scalar):
        for light in ((0.0, 0.0, 0.5, 1.0), (1e200, 0.0, 0.0, 1.0)):
            rgba = form(v, f, np.repeat(RED, 2, 0), np.eye(4), PIXEL_CAM, light=light, ambient=0.25)[0]
            assert tuple(rgba[8, 16]) == (50, 23, 8, 255)            # 50.25, 22.5, 8.25 (+ 0.5, floor)


# ------------------------------------------------------------------------------- tie-break
@pytest.mark.parametrize("flip", [False, True])
def test_shared_edge_goes_to_the_smaller_index_whatever_the_order(flip):
    images = []
    for swap in (False, True):
        (v, f), colors, (left, edge, right) = semu.tie_squares(swap, flip)
        assert np.array_equal(v.astype(np.float64), np.asarray(v, np.float64)) and len(f) == 4
        base = semu.render(v, f, colors, np.eye(4), PIXEL_CAM, ambient=1.0)
        for order in ([3, 2, 1, 0], [2, 0, 3, 1], [1, 3, 0, 2]):
            other = semu.render(v, f, colors, np.eye(4), PIXEL_CAM, ambient=1.0, order=order)
            assert all(np.array_equal(x, y) for x, y in zip(base, other))
        rgba, depth, index = base
        first, second = colors[0], colors[2]
        assert (index[edge] < 2).all() and (rgba[edge] == first).all()                      # the square that comes first in the mesh
        lo, hi = (right, left) if swap else (left, right)
        assert (rgba[lo] == first).all() and (rgba[hi] == second).all() and (index[hi] >= 2).all()
        assert (depth[left | edge | right] == F32(0.5)).all() and (index[~(left | edge | right)] == -1).all()
        images.append(rgba)
    # permuting the two squares changes who owns the edge, nothing else
    (_, _, (left, edge, right)) = semu.tie_squares(False, flip)
    assert np.array_equal(images[0][~edge], images[1][~edge]) and not np.array_equal(images[0][edge], images[1][edge])


# ------------------------------------------------------------------------------- cameras
def test_get_camera_pose_is_the_reference_formula():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(3)
    for _ in range(8):
        ax, ay, az = rng.uniform(-np.pi, np.pi, 3)
        radius, center = rng.uniform(0.2, 2.0), rng.uniform(-0.5, 0.5, 3)
        pose = visual.get_camera_pose(radius, center, ax, ay, az)
        rot = Rotation.from_euler("xyz", (ax, ay, az)).as_matrix()
        assert pose.shape == (4, 4) and np.allclose(pose[:3, :3], rot, atol=1e-14) and np.array_equal(pose[3], [0, 0, 0, 1])
        assert np.allclose(pose[:3, 3], rot @ [0, 0, radius] + center, atol=1e-14)
        at = visual.extrinsic_from_camera_pose(pose) @ np.r_[center, 1.0]                 # the centre: on the optical axis, `radius` away
        assert np.allclose(at, [0, 0, radius, 1], atol=1e-13)
    assert np.allclose(visual.get_camera_pose(0.5), [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5], [0, 0, 0, 1]])


def test_look_at_and_the_extrinsic_conversion():
    eye, target = np.array([0.4, -0.3, 0.5]), np.array([0.15, 0.15, 0.05])
    pose = visual.look_at(eye, target)
    R = pose[:3, :3]
    assert np.allclose(R.T @ R, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(R), 1.0) and np.allclose(pose[:3, 3], eye)
    assert np.allclose(-R[:, 2], (target - eye) / np.linalg.norm(target - eye))           # the camera looks down -z
    assert R[2, 1] > 0                                                                    # image up is world up
    E = visual.extrinsic_from_camera_pose(pose)
    assert np.allclose(E @ np.r_[target, 1.0], [0, 0, np.linalg.norm(target - eye), 1], atol=1e-13)
    assert np.allclose(E @ np.r_[eye, 1.0], [0, 0, 0, 1], atol=1e-13)
    assert (E @ np.r_[target + [0, 0, 0.1], 1.0])[1] < 0                                   # a point above the target: up in the image (y down)
    # the package's own view circle, written as a pose and converted back
    origin = np.eye(4)
    origin[:3, 3] = [0.15, 0.15, 0.0]
    ext = perception.camera_on_sphere(origin, 0.6, np.pi / 6, 0.5)
    cam_to_world = np.linalg.inv(ext) @ np.diag([1.0, -1.0, -1.0, 1.0])
    assert np.allclose(visual.extrinsic_from_camera_pose(cam_to_world), ext, atol=1e-13)
    with pytest.raises(ValueError):
        visual.look_at([0, 0, 1], [0, 0, 0], up=(0, 0, 1))


# ------------------------------------------------------------------------------- supersampling
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_supersample_centres_are_symmetric_about_the_pixel_centre(k):
    intr = perception.CameraIntrinsic(53, 37, 45.0, 44.0, 26.25, 18.5)
    for po in (0.0, 0.5):
        (W, H, fx, fy, cx, cy), pof = render.supersample_camera(intr, po, k)
        assert ((W, H, fx, fy, cx, cy), pof) == semu.supersample_camera(semu.SMALL, po, k) and (W, H) == (53 * k, 37 * k)
        for u in (0, 7, 52):
            centre = ((u + po) - 26.25) / 45.0
            fine = np.array([((k * u + i + pof) - cx) / fx for i in range(k)])
            assert np.allclose(fine.mean(), centre, atol=1e-15) and np.allclose(fine - centre, -(fine - centre)[::-1], atol=1e-15)
            assert np.allclose(np.diff(fine), 1.0 / (k * 45.0)) and abs(fine[0] - centre) < 0.5 / 45.0      # inside the footprint
    with pytest.raises(ValueError):
        render.supersample_camera(intr, 0.0, 5)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_downsample_arithmetic(k):
    rng = np.random.default_rng(k)
    img = rng.integers(0, 256, size=(2, 5 * k, 7 * k, 4), dtype=np.uint8)
    got = semu.downsample(img, k)
    assert got.shape == (2, 5, 7, 4) and got.dtype == np.uint8
    for v, u, c in ((0, 0, 0), (4, 6, 3), (2, 3, 1)):
        s = sum(int(img[1, k * v + j, k * u + i, c]) for j in range(k) for i in range(k))
        assert got[1, v, u, c] == (s + (k * k) // 2) // (k * k)
    assert np.array_equal(semu.downsample(np.full((4 * k, 4 * k, 4), 255, np.uint8), k), np.full((4, 4, 4), 255, np.uint8))
    if k == 1:
        assert np.array_equal(got, img)


# ------------------------------------------------------------------------------- PNG
def _decode_png(path):
    """inflate the IDAT chunk and undo filter 0: (H, W, C) uint8"""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(data):
        n, tag = struct.unpack(">I", data[at:at + 4])[0], data[at + 4:at + 8]
        body = data[at + 8:at + 8 + n]
        assert struct.unpack(">I", data[at + 8 + n:at + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        chunks.append((tag, body))
        at += 12 + n
    assert [t for t, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, kind, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and kind in (2, 6)
    C = 3 if kind == 2 else 4
    rows = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + W * C)
    assert (rows[:, 0] == 0).all()
    return rows[:, 1:].reshape(H, W, C)


@pytest.mark.parametrize("shape", [(1, 1, 3), (1, 1, 4), (37, 53, 3), (37, 53, 4)])
def test_write_png_round_trip(tmp_path, shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    path = visual.write_png(tmp_path / "a.png", img)
    assert path == str(tmp_path / "a.png") and np.array_equal(_decode_png(path), img)


@pytest.mark.parametrize("shape", [(1, 1, 3), (37, 53, 3), (37, 53, 4)])
def test_write_png_decodes_with_pil(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(sum(shape)).integers(0, 256, size=shape, dtype=np.uint8)
    with Image.open(visual.write_png(tmp_path / "a.png", img)) as im:
        assert im.mode == ("RGB" if shape[2] == 3 else "RGBA") and np.array_equal(np.asarray(im), img)


def test_write_png_rejects_other_arrays(tmp_path):
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((4, 4, 2), np.uint8), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            visual.write_png(tmp_path / "b.png", bad)


# ------------------------------------------------------------------------------- ABI validation without a device
_BUF = (ctypes.c_double * 256)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 30
IDENT = tuple(np.eye(4).reshape(-1))
CAM2 = (500.0, 500.0, 32.0, 24.0) * 2
LIGHT2 = (0.0, 0.0, 0.0, 1.0) * 2


def _arr(values, ctype):
    return NUL if values is None else (ctype * len(values))(*values)


def _color(vertices=A, voffs=(0, 8), triangles=A, toffs=(0, 12), colors=A, view_offs=(0, 2), ext=IDENT * 2, cam=CAM2, lights=LIGHT2,
           ambient=0.3, bg=(255, 255, 255, 255), B=1, W=64, H=48, near=0.1, far=2.0, po=0.0, rgba=A, depth=A, index=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_color_render(vertices, _arr(voffs, ctypes.c_int32), triangles, _arr(toffs, ctypes.c_int32), colors,
                                         _arr(view_offs, ctypes.c_int32), _arr(ext, ctypes.c_double), _arr(cam, ctypes.c_double),
                                         _arr(lights, ctypes.c_double), ambient, _arr(bg, ctypes.c_uint8), B, W, H, near, far, po,
                                         rgba, depth, index, ws, ws_bytes, NUL)


def _with(seq, i, value):
    seq = list(seq)
    seq[i] = value
    return tuple(seq)


@pytest.mark.parametrize("kwargs, code", [
    (dict(B=-1), -1), (dict(B=_capi.MAX_SCENES + 1), -7),
    (dict(W=0), -1), (dict(H=0), -1), (dict(W=4097), -1), (dict(H=4097), -1),
    (dict(near=0.0), -1), (dict(near=float("nan")), -1), (dict(far=0.1), -1), (dict(far=float("inf")), -1), (dict(po=float("nan")), -1),
    (dict(voffs=None), -1), (dict(toffs=None), -1), (dict(view_offs=None), -1),
    (dict(voffs=(1, 8)), -1), (dict(toffs=(0, -1)), -1), (dict(view_offs=(0, -2)), -1),
    (dict(B=2, voffs=(0, 8, 8), toffs=(0, 12, 6), view_offs=(0, 1, 2)), -1),
    (dict(W=4096, H=4096, view_offs=(0, 128), ext=IDENT * 128, cam=CAM2 * 64, lights=LIGHT2 * 64), -1),        # n W H = 2^31
    (dict(vertices=NUL), -1), (dict(triangles=NUL), -1), (dict(ext=None), -1), (dict(cam=None), -1), (dict(ws=NUL), -1),
    (dict(cam=_with(CAM2, 0, 0.0)), -1), (dict(cam=_with(CAM2, 7, float("inf"))), -1), (dict(ext=_with(IDENT * 2, 3, float("nan"))), -1),
    (dict(ambient=-0.01), -1), (dict(ambient=1.01), -1), (dict(ambient=float("nan")), -1),
    (dict(lights=_with(LIGHT2, 2, float("nan"))), -1), (dict(lights=_with(LIGHT2, 7, float("inf"))), -1),
    (dict(colors=NUL), -1), (dict(colors=ctypes.c_void_p(A.value + 2)), -1),
    (dict(rgba=NUL), -6), (dict(ws_bytes=100), -4),
    (dict(B=0), 0), (dict(B=0, voffs=None, toffs=None, view_offs=None, ext=None, cam=None, lights=None, vertices=NUL, triangles=NUL,
                          colors=NUL, rgba=NUL), 0),
    (dict(view_offs=(0, 0), ext=None, cam=None, lights=None, rgba=NUL, ws=NUL), 0),                             # no views: nothing to do
    (dict(voffs=(0, 0), toffs=(0, 0), colors=NUL, vertices=NUL, triangles=NUL, rgba=NUL), -6),                  # an empty mesh needs no colours
])
def test_color_render_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _color(**kwargs) == code


@pytest.mark.parametrize("kwargs, code", [
    (dict(n=-1), -1), (dict(k=0), -1), (dict(k=5), -1), (dict(W=0), -1), (dict(H=0), -1), (dict(W=4097), -1), (dict(H=4097), -1),
    (dict(n=8, W=4096, H=4096, k=4), -1), (dict(src=NUL), -1), (dict(dst=NUL), -6), (dict(n=0, src=NUL, dst=NUL), 0),
])
def test_image_downsample_rejects_invalid_arguments_without_a_device(kwargs, code):
    args = dict(src=A, dst=A, n=1, W=8, H=8, k=2)
    args.update(kwargs)
    assert _capi.lib().giga_image_downsample(args["src"], args["dst"], args["n"], args["W"], args["H"], args["k"], NUL) == code


def test_color_render_is_exported_and_declared():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_color_render", "giga_color_render_workspace_bytes", "giga_image_downsample"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    assert _capi.DOWNSAMPLE_MAX_K == int(hdr.split("#define GIGA_DOWNSAMPLE_MAX_K")[1].split()[0]) == 4
    assert L.giga_color_render_workspace_bytes(0, 6, 8, 12) == 0 and L.giga_color_render_workspace_bytes(1, -1, 8, 12) == 0
    # the depth render's workspace and four doubles per view for the lights
    assert L.giga_color_render_workspace_bytes(4, 24, 100, 200) >= L.giga_depth_render_workspace_bytes(4, 24, 100, 200) + 24 * 4 * 8


# ------------------------------------------------------------------------------- host logic
def test_color_rendering_needs_a_device_and_checks_its_arguments():
    import torch
    import giga_amd
    v, f = remu.plane_mesh(0.5, 0.1)
    colors = np.repeat(RED, 2, 0)
    with pytest.raises(_capi.GigaHipError):
        render.render_color(torch.from_numpy(v), torch.from_numpy(f), colors, render.sim_intrinsic(), [np.eye(4)], device="cpu")
    with pytest.raises(ValueError):
        render.render_color_batch([(v, f)], [colors, colors], render.sim_intrinsic(), [[np.eye(4)]])
    assert render._lights(None, 3).tolist() == [[0.0, 0.0, 0.0, 1.0]] * 3 and render._lights((1, 2, 3, 0), 2).shape == (2, 4)
    with pytest.raises(ValueError):
        render._lights(np.zeros((3, 4)), 2)
    assert giga_amd.render_color is render.render_color and giga_amd.render_mesh is visual.render_mesh
    assert giga_amd.write_png is visual.write_png and giga_amd.get_camera_pose is visual.get_camera_pose
    assert callable(visual.Scene.render) and callable(visual.Scene.save_image) and callable(render.Camera.render_rgbd)
