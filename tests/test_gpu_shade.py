"""GPU tests of the colour renderer (csrc/giga_render.hip: giga_color_render, giga_image_downsample) and of what giga_amd.render and
giga_amd.visual build on it.  Triangle index and depth are compared BYTE FOR BYTE with the numpy restatement of
tests/shade_emu.py, whose two forms agree in bytes on these very scenes (tests/test_shade_host.py).  So is the colour: the bound
this started from was one level per channel on at most 0.5 % of the hit pixels (the square root and the floor are the operations
of the shade whose device implementation the restatement takes on trust); the device differed on 0 pixels of every scene, and the
check was tightened to equality."""
import functools

import numpy as np
import pytest
import torch

import render_emu as remu
import shade_emu as semu
import tsdf_emu as emu
from giga_amd import _capi, perception, render, visual

pytestmark = pytest.mark.gpu
F32 = np.float32
FAR = 2.0
SIZE = 0.3


def dev():
    return torch.device("cuda:0")


def intrinsic_of(K):
    return perception.CameraIntrinsic(*K)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's (rgba, depth, index) of a case: computed once, shared, never changed"""
    case = {"full": semu.FULL, "super": semu.SUPER}.get(name) or semu.CASES[name]
    out = semu.render_case(case())
    for a in out:
        a.setflags(write=False)
    return out


def gpu_render(case, **extra):
    (v, f), colors, K, ext, kw = case
    kw = dict(kw, **extra)
    return render.render_color(v, f, colors, intrinsic_of(K), ext, return_buffers=True, device=dev(), **kw)


def check_index_and_depth(got_depth, got_index, want, what):
    _, depth, index = want
    gd, gi = got_depth.cpu().numpy(), got_index.cpu().numpy()
    assert gd.shape == depth.shape and gd.dtype == F32 and gi.shape == index.shape and gi.dtype == np.int32
    bad_i, bad_d = int((gi != index).sum()), int((gd.view(np.uint32) != depth.view(np.uint32)).sum())
    print(f"{what}: {bad_i} indices and {bad_d} depth words of {index.size} differ; {int((index >= 0).sum())} pixels hit")
    assert bad_i == 0 and bad_d == 0, what


def check_colour(got, want_rgba, hit, what):
    """every byte equal"""
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.shape == want_rgba.shape and g.dtype == np.uint8
    diff = np.abs(g.astype(np.int16) - want_rgba.astype(np.int16))
    pixels = int(diff.max(axis=-1).astype(bool).sum())
    print(f"{what}: colour differs on {pixels} of {int(hit.sum())} hit pixels, by at most {int(diff.max()) if diff.size else 0} levels")
    assert pixels == 0 and np.array_equal(g, want_rgba), what


@pytest.mark.parametrize("name", list(semu.CASES))
def test_color_render_matches_the_restatement(name):
    case = semu.CASES[name]()
    (v, f), colors, K, ext, kw = case
    want = reference(name)
    stats = {}
    rgba, depth, index = gpu_render(case, stats=stats)
    assert rgba.is_cuda and rgba.shape == (len(ext), K[1], K[0], 4) and rgba.dtype == torch.uint8
    check_index_and_depth(depth, index, want, name)
    check_colour(rgba, want[0], want[2] >= 0, name)
    # the depth render of the same call: the same bytes
    plain = render.render_depth(v, f, intrinsic_of(K), ext, near=kw.get("near", 0.1), far=kw.get("far", FAR),
                                pixel_offset=kw.get("pixel_offset", 0.0), device=dev())
    assert torch.equal(plain.view(torch.int32), depth.view(torch.int32))
    # without the optional buffers the colours are the same
    assert torch.equal(render.render_color(v, f, colors, intrinsic_of(K), ext, device=dev(), **kw), rgba)
    if name == "six-37x53-plane-boxes":
        assert len(f) % 256 != 0 and (want[2] >= 0).all()
    if name == "tile-icosphere-1280":
        assert stats["tile_pairs"] >= 1280 > 384                     # one tile keeps every triangle: the list is flushed several times
    if name.startswith("tie-squares"):
        edge = semu.tie_squares(False, False)[2][1]
        gi = index[0].cpu().numpy()
        assert (gi[edge] < 2).all() and (gi[edge] >= 0).all()        # the shared edge: the square that comes first
    if name == "empty-mesh":
        assert bool((index == -1).all()) and (rgba.cpu().numpy() == np.array([9, 8, 7, 0], np.uint8)).all() and bool((depth == FAR).all())
    if name == "nan-vertex-bad-index":
        gi = index.cpu().numpy()
        assert set(np.unique(gi)) <= {-1, 2, 3}                      # only the two finite, in-range triangles ever win
    if name == "ambient-1":
        hit = want[2] >= 0
        assert np.array_equal(rgba.cpu().numpy()[hit][:, :3], colors[want[2][hit]][:, :3])           # k = 1: the faces' own colours
    if name == "behind-the-camera":
        assert bool((index[0, 12] == 0).all()) and bool((index[0, :10] == -1).all())


def test_tie_break_images_do_not_depend_on_the_face_order():
    for flip in (False, True):
        imgs = []
        for swap in (False, True):
            (v, f), colors, (left, edge, right) = semu.tie_squares(swap, flip)
            want = semu.render(v, f, colors, np.eye(4), semu.PIXEL_CAM, ambient=1.0)
            rgba, depth, index = render.render_color(v, f, colors, intrinsic_of(semu.PIXEL_CAM), [np.eye(4)], ambient=1.0,
                                                     return_buffers=True, device=dev())
            assert np.array_equal(rgba[0].cpu().numpy(), want[0]) and np.array_equal(index[0].cpu().numpy(), want[2])
            perm = np.array([3, 1, 0, 2])                            # the same four triangles in another order: the same picture
            again = render.render_color(v, f[perm], colors[perm], intrinsic_of(semu.PIXEL_CAM), [np.eye(4)], ambient=1.0, device=dev())
            g = rgba[0].cpu().numpy()
            assert np.array_equal(again[0].cpu().numpy()[~edge], g[~edge])
            assert (g[edge] == colors[0]).all()
            imgs.append(g)
        assert np.array_equal(imgs[0][~edge], imgs[1][~edge])


def test_ragged_batch_equals_single_calls_and_repeats():
    K = semu.SMALL
    counts = (6, 1, 3, 0)
    meshes = [semu.plane_boxes(4), remu.icosphere((0.15, 0.15, 0.1), 0.05, 1), semu.plane_boxes(5), semu.plane_boxes(6)]
    colors = [semu.random_colors(len(m[1]), 10 + b) for b, m in enumerate(meshes)]
    exts = [emu.six_views(SIZE, n, 6) if n else np.zeros((0, 4, 4)) for n in counts]
    lights = np.concatenate([np.tile([[0.1, 0.2, -0.3, 1.0]], (6, 1)), [[0, 0, 0, 1.0]], np.tile([[0.3, 0.1, -1.0, 0.0]], (3, 1))])
    rgba, offs, depth, index = render.render_color_batch(meshes, colors, intrinsic_of(K), exts, lights=lights, return_buffers=True, device=dev())
    again = render.render_color_batch(meshes, colors, intrinsic_of(K), exts, lights=lights, return_buffers=True, device=dev())
    assert offs.tolist() == [0, 6, 7, 10, 10] and rgba.shape == (10, K[1], K[0], 4)
    assert torch.equal(rgba, again[0]) and torch.equal(depth, again[2]) and torch.equal(index, again[3])
    for b, (m, c, e) in enumerate(zip(meshes, colors, exts)):
        if not len(e):
            continue
        one = render.render_color(m[0], m[1], c, intrinsic_of(K), e, lights=lights[offs[b]:offs[b + 1]], return_buffers=True, device=dev())
        for got, want in zip(one, (rgba, depth, index)):
            assert torch.equal(got, want[offs[b]:offs[b + 1]])
    want = semu.render_views(*meshes[2], colors[2], exts[2], K, lights=lights[7:10])
    check_index_and_depth(depth[7:10], index[7:10], want, "batch scene 2")
    check_colour(rgba[7:10], want[0], want[2] >= 0, "batch scene 2")
    r0, o0 = render.render_color_batch([], [], intrinsic_of(K), [], device=dev())
    assert r0.shape == (0, K[1], K[0], 4) and o0.tolist() == [0]


def test_one_view_at_the_camera_resolution():
    case = semu.FULL()
    rgba, depth, index = gpu_render(case)
    want = reference("full")
    check_index_and_depth(depth, index, want, "480x640 one view")
    check_colour(rgba, want[0], want[2] >= 0, "480x640 one view")


@pytest.mark.parametrize("k", [2, 3])
def test_supersampling_equals_the_downsampled_fine_restatement(k):
    (v, f), colors, K, ext, kw = semu.SUPER()
    Kf, po = semu.supersample_camera(K, 0.0, k)
    fine = semu.render_views(v, f, colors, ext, Kf, pixel_offset=po)
    rgba, depth, index = render.render_color(v, f, colors, intrinsic_of(K), ext, supersample=k, return_buffers=True, device=dev())
    assert rgba.shape == (len(ext), K[1], K[0], 4) and depth.shape == (len(ext), k * K[1], k * K[0])
    check_index_and_depth(depth, index, fine, f"supersample {k}, fine buffers")
    hit = semu.downsample(np.repeat((fine[2] >= 0)[..., None], 4, -1).astype(np.uint8) * 255, k)[..., 0] > 0
    check_colour(rgba, semu.downsample(fine[0], k), hit, f"supersample {k}")
    one = render.render_color(v, f, colors, intrinsic_of(K), ext, device=dev())
    assert not torch.equal(one, rgba)                                # edges are blended


@pytest.mark.parametrize("k, n, H, W", [(1, 2, 5, 7), (2, 3, 37, 53), (3, 1, 16, 33), (4, 2, 9, 17)])
def test_image_downsample_is_exact(k, n, H, W):
    img = np.random.default_rng(k).integers(0, 256, size=(n, k * H, k * W, 4), dtype=np.uint8)
    got = render.downsample(torch.from_numpy(img).to(dev()), k)
    assert got.shape == (n, H, W, 4) and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), semu.downsample(img, k))
    with pytest.raises(ValueError):
        render.downsample(torch.zeros((1, 5, 6, 4), dtype=torch.uint8, device=dev()), 4)


# ------------------------------------------------------------------------------------------------ the public interface
def hand_built_scene():
    v, f = remu.box_mesh((0.1, 0.1, 0.05), (0.2, 0.2, 0.12))
    box = visual.ColoredMesh(v, f, np.tile(np.array([[180, 60, 40, 255]], np.uint8), (len(f), 1)))
    scene = visual.Scene(box)
    grasp = {"rotation": np.array([0.0, 0.0, 0.0, 1.0]), "translation": np.array([0.15, 0.15, 0.16]), "width": 0.08}
    scene.add_geometry(visual.grasp2mesh(grasp), "grasp_0")
    return scene


def test_render_mesh_and_scene_render(tmp_path):
    scene = hand_built_scene()
    K = (160, 120, 135.0, 135.0, 80.0, 60.0)
    pose = visual.look_at([0.15, -0.35, 0.4], [0.15, 0.15, 0.1])
    img = scene.render(pose, intrinsic=intrinsic_of(K), ambient=1.0)
    assert isinstance(img, np.ndarray) and img.shape == (120, 160, 3) and img.dtype == np.uint8
    flat = img.reshape(-1, 3)
    for colour in ((255, 255, 255), visual.GRIPPER_COLOR[:3], (180, 60, 40)):                     # background, gripper, box
        assert (flat == np.array(colour, np.uint8)).all(axis=1).any(), colour
    assert np.array_equal(img, visual.render_mesh(scene, pose, intrinsic=intrinsic_of(K), ambient=1.0))
    ext = visual.extrinsic_from_camera_pose(pose)
    direct = render.render_color(scene.vertices, scene.faces, scene.face_colors, intrinsic_of(K), [ext], ambient=1.0, device=dev())
    assert np.array_equal(direct[0, :, :, :3].cpu().numpy(), img)
    # a light of its own: a point light at light_pose's origin, in the camera frame
    light_pose = visual.get_camera_pose(0.5, (0.15, 0.15, 0.1), ax=0.3)
    lit = visual.render_mesh(scene, pose, light_pose, intrinsic=intrinsic_of(K))
    at = ext @ np.r_[light_pose[:3, 3], 1.0]
    direct = render.render_color(scene.vertices, scene.faces, scene.face_colors, intrinsic_of(K), [ext], lights=(at[0], at[1], at[2], 1.0),
                                 device=dev())
    assert np.array_equal(direct[0, :, :, :3].cpu().numpy(), lit) and not np.array_equal(lit, img)
    # the default view (the simulated camera's side view) and the file
    path = scene.save_image(tmp_path / "plan.png", intrinsic=intrinsic_of(K))
    default = scene.render(intrinsic=intrinsic_of(K))
    side = render.acquire_extrinsics(1, sideview=True)[0]
    direct = render.render_color(scene.vertices, scene.faces, scene.face_colors, intrinsic_of(K), [side], device=dev())
    assert np.array_equal(direct[0, :, :, :3].cpu().numpy(), default) and (default != 255).any()
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (160, 120)
    n = struct.unpack(">I", data[33:37])[0]
    assert data[37:41] == b"IDAT"
    rows = np.frombuffer(zlib.decompress(data[41:41 + n]), np.uint8).reshape(120, 1 + 160 * 3)
    assert (rows[:, 0] == 0).all() and np.array_equal(rows[:, 1:].reshape(120, 160, 3), default)
    assert scene.render().shape == (480, 640, 3)                     # the simulated camera by default


def test_camera_render_rgbd():
    (v, f), colors, K, ext, kw = semu.CASES["six-37x53-plane-boxes"]()
    cam = render.Camera(intrinsic_of(K), 0.1, FAR)
    vt, ft = torch.from_numpy(v).to(dev()), torch.from_numpy(f).to(dev())
    rgb, depth = cam.render_rgbd(ext[2], vt, ft, torch.from_numpy(colors).to(dev()))
    assert rgb.shape == (K[1], K[0], 3) and rgb.dtype == torch.uint8 and depth.shape == (K[1], K[0]) and depth.dtype == torch.float32
    assert torch.equal(depth.view(torch.int32), cam.render(ext[2], vt, ft).view(torch.int32))
    want = reference("six-37x53-plane-boxes")
    check_colour(rgb, want[0][2, :, :, :3], want[2][2] >= 0, "render_rgbd")


def test_color_rendering_rejects_bad_arguments_on_the_device():
    (v, f), colors, K, ext, kw = semu.CASES["ambient-0"]()
    for bad in (dict(ambient=1.5), dict(lights=(0.0, float("nan"), 0.0, 1.0)), dict(near=0.0)):
        with pytest.raises(_capi.GigaHipError):
            render.render_color(v, f, colors, intrinsic_of(K), ext, device=dev(), **bad)
    with pytest.raises(ValueError):
        render.render_color(v, f, colors[:-1], intrinsic_of(K), ext, device=dev())
