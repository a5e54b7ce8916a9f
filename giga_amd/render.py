"""Depth images and occupancy labels from triangle meshes on the device: what the reference derives from its simulated scene.

`Camera.render` / `render_depth` / `render_depth_batch` are the depth half of `btsim.Camera.render` (reference
src/vgn/utils/btsim.py:276-337, PyBullet there) through `giga_depth_render` (csrc/giga_render.hip; semantics in
include/giga_hip.h): a double-precision watertight ray / triangle test per pixel, `far` where nothing is hit.  `acquire_tsdf` is
`ClutterRemovalSim.acquire_tsdf` (simulation.py:145-186) on a scene mesh, `write_raw_scenes` the raw files `construct_dataset`
consumes, `sample_iou_points` / `save_occ` the occupancy labels of utils/implicit.py:78-90 and scripts/save_occ_data_parallel.py
on top of `giga_mesh_contains`.  Meshes are `(vertices, faces)` pairs of numpy arrays or device tensors (or objects with these
attributes); loading mesh files stays with the caller.  There is no CPU path: CPU tensors raise `GigaHipError`.

The reference's depth noise (simulation.py:176, `--add-noise`) is the `noise=` argument of `acquire_tsdf` / `acquire_tsdfs`: a
`giga_amd.noise.DepthNoise`, applied on the device between rendering and fusion.

`render_color` / `render_color_batch` / `Camera.render_rgbd` are the RGB half, through `giga_color_render`: the depth renderer's
visibility with the winning triangle kept (smallest z, then smallest index), and a flat, two-sided shade of the per-face colours
under one light per view and an ambient term, all in double (include/giga_hip.h has the arithmetic).  `supersample=k` renders the
k x k sample centres of every pixel and box-filters them with `giga_image_downsample`.  The shading model is the project's own,
not PyBullet's or pyrender's: agreement with either is not claimed.

Not reproduced: PyBullet's fill rule at silhouettes, its z-buffer quantisation, its lighting model; smooth shading, textures,
shadows and transparency."""
import json
import os
import time
from pathlib import Path

import numpy as np
import torch

from . import _capi, perception, ragged
from .eval import mesh_contains_batch

SIM_INTRINSIC = (640, 480, 540.0, 540.0, 320.0, 240.0)       # simulation.py:38: width, height, fx, fy, cx, cy
SIM_NEAR, SIM_FAR = 0.1, 2.0                                  # simulation.py:39


def sim_intrinsic():
    return perception.CameraIntrinsic(*SIM_INTRINSIC)


def scene_mesh(mesh_pose_list):
    """[(vertices (n, 3), faces (m, 3), scale, pose 4x4), ...] -> one (vertices float32, faces int32) pair: `scale` then `pose`
    applied in float64, faces re-based: the array form of get_scene_from_mesh_pose_list (utils/implicit.py:53-76)."""
    verts, faces, base = [], [], 0
    for v, f, scale, pose in mesh_pose_list:
        v = np.asarray(v, np.float64).reshape(-1, 3) * np.asarray(scale, np.float64)
        pose = np.asarray(pose, np.float64).reshape(4, 4)
        v = v @ pose[:3, :3].T + pose[:3, 3]
        verts.append(v.astype(np.float32))
        faces.append(np.asarray(f, np.int64).reshape(-1, 3) + base)
        base += len(v)
    if not verts:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


# ------------------------------------------------------------------------------------------------ rendering
def render_depth_batch(meshes, intrinsic, extrinsics_batches, near=SIM_NEAR, far=SIM_FAR, pixel_offset=0.0, device=None, stats=None):
    """B scenes with ragged view counts in one launch: meshes[b] seen from extrinsics_batches[b] (any extrinsic form).
    Returns (depth (n_total, H, W) float32 device tensor, view_offsets (B + 1) int32): view k of scene b is image
    view_offsets[b] + k, the layout `perception.integrate_batch` consumes.  stats (a dict) receives 'tile_pairs', the number of
    (triangle, 16x16 tile) pairs that survived the kernel's culling (this reads the workspace back: a synchronisation)."""
    if len(extrinsics_batches) != len(meshes):
        raise ValueError("one list of extrinsics per mesh")
    B = len(meshes)
    dev = _capi.hip_device(*ragged.mesh_arrays(meshes), device=device, what="depth rendering runs on a HIP device")
    H, W = int(intrinsic.height), int(intrinsic.width)
    view_offsets = ragged.offsets([len(e) for e in extrinsics_batches])
    n = int(view_offsets[-1])
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    if B == 0 or n == 0:
        return depth, view_offsets
    v, vo, f, fo = ragged.pack_meshes(meshes, dev)
    ext = np.ascontiguousarray(np.stack([perception.extrinsic_matrix(e) for batch in extrinsics_batches for e in batch]).reshape(n, 16))
    cam = np.ascontiguousarray(np.tile(np.array([intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy], np.float64), (n, 1)))
    ws = _capi.workspace("giga_depth_render", dev, B, n, int(vo[-1]), int(fo[-1]))
    _capi.call("giga_depth_render", dev, v, vo, f, fo, view_offsets, ext, cam, B, W, H, float(near), float(far), float(pixel_offset),
               depth, ws, ws.numel())
    if stats is not None:
        stats["tile_pairs"] = stats.get("tile_pairs", 0) + int(ws[:8].cpu().numpy().view(np.uint64)[0])
    return depth, view_offsets


def render_depth(vertices, faces, intrinsic, extrinsics, near=SIM_NEAR, far=SIM_FAR, pixel_offset=0.0, device=None):
    """(n, H, W) float32 device tensor: one mesh seen from n extrinsics."""
    return render_depth_batch([(vertices, faces)], intrinsic, [list(extrinsics)], near, far, pixel_offset, device)[0]


HEADLIGHT = (0.0, 0.0, 0.0, 1.0)                              # a point light at the camera


def supersample_camera(intrinsic, pixel_offset, k):
    """((k W, k H, k fx, k fy, k cx, k cy), k (pixel_offset - 0.5) + 0.5): the camera whose pixels are the k x k sample centres
    inside each pixel's footprint of `intrinsic`, symmetric about the pixel's centre.  k = 1 changes nothing."""
    k = int(k)
    if not 1 <= k <= _capi.DOWNSAMPLE_MAX_K:
        raise ValueError(f"supersample is 1 .. {_capi.DOWNSAMPLE_MAX_K}, not {k}")
    W, H = int(intrinsic.width), int(intrinsic.height)
    if k == 1:
        return (W, H, float(intrinsic.fx), float(intrinsic.fy), float(intrinsic.cx), float(intrinsic.cy)), float(pixel_offset)
    return ((k * W, k * H, k * float(intrinsic.fx), k * float(intrinsic.fy), k * float(intrinsic.cx), k * float(intrinsic.cy)),
            k * (float(pixel_offset) - 0.5) + 0.5)


def downsample(rgba, k):
    """(n, k H, k W, 4) uint8 device tensor -> (n, H, W, 4): the exact k x k box filter of giga_image_downsample."""
    n, Hk, Wk = int(rgba.shape[0]), int(rgba.shape[1]), int(rgba.shape[2])
    k = int(k)
    if not 1 <= k <= _capi.DOWNSAMPLE_MAX_K or Hk % k or Wk % k or rgba.dim() != 4 or rgba.shape[3] != 4 or rgba.dtype != torch.uint8:
        raise ValueError(f"downsample takes (n, k H, k W, 4) uint8 and k in 1 .. {_capi.DOWNSAMPLE_MAX_K}")
    dev = _capi.hip_device(rgba, what="images are filtered on a HIP device")
    src = rgba.contiguous()
    dst = torch.empty((n, Hk // k, Wk // k, 4), dtype=torch.uint8, device=dev)
    if n:
        _capi.call("giga_image_downsample", dev, src, dst, n, Wk // k, Hk // k, k)
    return dst


def _lights(lights, n):
    """None, one (lx, ly, lz, lw) or one per view -> (n, 4) float64"""
    a = np.asarray(HEADLIGHT if lights is None else lights, np.float64)
    if a.shape == (4,):
        a = np.tile(a, (n, 1))
    if a.shape != (n, 4):
        raise ValueError(f"lights: one (lx, ly, lz, lw) or one per view ({n}), not an array of shape {a.shape}")
    return np.ascontiguousarray(a)


def render_color_batch(meshes, face_colors, intrinsic, extrinsics_batches, lights=None, ambient=0.3, background=(255, 255, 255, 255),
                       near=SIM_NEAR, far=SIM_FAR, pixel_offset=0.0, supersample=1, return_buffers=False, device=None, stats=None):
    """Shaded images of B coloured scenes with ragged view counts in one launch of giga_color_render (flat, two-sided shading of
    the face colours: the project's own model, see include/giga_hip.h; not pyrender's).  face_colors[b]: (F_b, 4) uint8 RGBA per
    face of meshes[b] (numpy or device tensor).  lights: None (the headlight), one (lx, ly, lz, lw) in the camera frame, or one per
    view: lw = 1 a point light at that position, lw = 0 a direction towards the light.  supersample = k renders k x k samples per
    pixel and box-filters them.
    Returns (rgba (n, H, W, 4) uint8 device tensor, view_offsets); with return_buffers also depth (n, kH, kW) float32 and the
    winning triangle's index in its scene (n, kH, kW) int32, -1 for none, both at the rendered (fine) resolution.  stats: as for
    `render_depth_batch`."""
    if len(extrinsics_batches) != len(meshes) or len(face_colors) != len(meshes):
        raise ValueError("one list of extrinsics and one colour array per mesh")
    B = len(meshes)
    dev = _capi.hip_device(*ragged.mesh_arrays(meshes), *face_colors, device=device, what="colour rendering runs on a HIP device")
    k = int(supersample)
    (W, H, fx, fy, cx, cy), po = supersample_camera(intrinsic, pixel_offset, k)
    view_offsets = ragged.offsets([len(e) for e in extrinsics_batches])
    n = int(view_offsets[-1])
    bg = np.ascontiguousarray(np.asarray(background).reshape(4), np.uint8)
    if not np.array_equal(bg, np.asarray(background).reshape(4)):
        raise ValueError("background is four bytes, RGBA")
    fine = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev) if return_buffers else None
    index = torch.empty((n, H, W), dtype=torch.int32, device=dev) if return_buffers else None
    if B and n:
        v, vo, f, fo = ragged.pack_meshes(meshes, dev)
        col, co = ragged.pack(face_colors, dev, torch.uint8, cols=4)
        if not np.array_equal(co, fo):
            raise ValueError("one colour per face")
        ext = np.ascontiguousarray(np.stack([perception.extrinsic_matrix(e) for batch in extrinsics_batches for e in batch]).reshape(n, 16))
        cam = np.ascontiguousarray(np.tile(np.array([fx, fy, cx, cy], np.float64), (n, 1)))
        ws = _capi.workspace("giga_color_render", dev, B, n, int(vo[-1]), int(fo[-1]))
        _capi.call("giga_color_render", dev, v, vo, f, fo, col, view_offsets, ext, cam, _lights(lights, n), float(ambient), bg, B, W, H,
                   float(near), float(far), po, fine, depth, index, ws, ws.numel())
        if stats is not None:
            stats["tile_pairs"] = stats.get("tile_pairs", 0) + int(ws[:8].cpu().numpy().view(np.uint64)[0])
    rgba = downsample(fine, k) if k > 1 else fine
    return (rgba, view_offsets, depth, index) if return_buffers else (rgba, view_offsets)


def render_color(vertices, faces, face_colors, intrinsic, extrinsics, **kwargs):
    """`render_color_batch` for one mesh seen from n extrinsics: (n, H, W, 4) uint8 device tensor (with return_buffers: that,
    depth and triangle index)."""
    out = render_color_batch([(vertices, faces)], [face_colors], intrinsic, [list(extrinsics)], **kwargs)
    return (out[0], out[2], out[3]) if kwargs.get("return_buffers") else out[0]


class Camera(object):
    """btsim.Camera (btsim.py:276-337): the mesh is passed in instead of living in a physics world.  `render` returns the depth
    image, `render_rgbd` the (rgb, depth) pair of the reference's `render`."""

    def __init__(self, intrinsic, near, far):
        self.intrinsic = intrinsic
        self.near = near
        self.far = far

    def render_rgbd(self, extrinsic, vertices, faces, face_colors, pixel_offset=0.0, device=None, **shade):
        """(rgb (H, W, 3) uint8, depth (H, W) float32) device tensors; shade: lights, ambient, background of `render_color_batch`.
        The depth is `render`'s, byte for byte."""
        rgba, depth, _ = render_color(vertices, faces, face_colors, self.intrinsic, [extrinsic], near=self.near, far=self.far,
                                      pixel_offset=pixel_offset, return_buffers=True, device=device, **shade)
        return rgba[0, :, :, :3], depth[0]

    def render(self, extrinsic, vertices, faces, pixel_offset=0.0, device=None):
        """extrinsic: the transform from the world to the camera frame, T_cam_world (any extrinsic form).
        Returns the depth image (H, W) as a float32 device tensor."""
        return render_depth(vertices, faces, self.intrinsic, [extrinsic], self.near, self.far, pixel_offset, device)[0]


# ------------------------------------------------------------------------------------------------ acquire_tsdf
def acquire_extrinsics(n, N=None, size=0.3, sideview=False):
    """(n, 4, 4) extrinsics of simulation.py:155-169: top view, n of N cameras on a circle about (size/2, size/2, 0) at
    theta = pi/6, r = 2 size; sideview, one camera about (size/2, size/2, size/3) at theta = pi/3, phi = -pi/2."""
    origin = np.eye(4)
    if sideview:
        origin[:3, 3] = [size / 2, size / 2, size / 3]
        theta = np.pi / 3.0
    else:
        origin[:3, 3] = [size / 2, size / 2, 0.0]
        theta = np.pi / 6.0
    r = 2.0 * size
    N = N if N else n
    if sideview:
        assert n == 1
        phi_list = [-np.pi / 2.0]
    else:
        phi_list = 2.0 * np.pi * np.arange(n) / N
    return np.stack([perception.camera_on_sphere(origin, r, theta, phi) for phi in phi_list]).reshape(-1, 4, 4)


def acquire_tsdf(vertices, faces, n, N=None, resolution=40, size=0.3, sideview=False, lower=None, upper=None, device=None, noise=None):
    """simulation.py:145-186 on a scene mesh: render n depth images with the reference's camera, integrate them into a volume of
    `resolution` and into a second one of 120.  Returns (TSDFVolume, pc, timing): pc the zero-crossing cloud of the second volume
    ((m, 3) float32 device tensor), cropped to lower <= p <= upper when both are given; timing the wall time of the integration
    into the first volume.  noise: a `giga_amd.noise.DepthNoise` applied to the rendered images (view k has the image id k) before
    BOTH volumes integrate them, as simulation.py:172-181 does; None leaves them as rendered.  The images never leave the device."""
    intrinsic = sim_intrinsic()
    extrinsics = acquire_extrinsics(n, N, size, sideview)
    depth = render_depth(vertices, faces, intrinsic, extrinsics, SIM_NEAR, SIM_FAR, 0.0, device)
    if noise is not None:
        depth = noise.apply(depth)
    tsdf = perception.TSDFVolume(size, resolution, depth.device)
    high_res_tsdf = perception.TSDFVolume(size, 120, depth.device)
    torch.cuda.synchronize(depth.device)
    tic = time.time()
    tsdf.integrate_views(depth, intrinsic, extrinsics)
    torch.cuda.synchronize(depth.device)
    timing = time.time() - tic
    high_res_tsdf.integrate_views(depth, intrinsic, extrinsics)
    pc = high_res_tsdf.get_cloud()
    if lower is not None and upper is not None:
        lo = torch.as_tensor(np.asarray(lower, np.float64), device=pc.device)
        hi = torch.as_tensor(np.asarray(upper, np.float64), device=pc.device)
        p = pc.double()
        pc = pc[((p >= lo) & (p <= hi)).all(dim=1)]         # o3d's AxisAlignedBoundingBox crop keeps min <= p <= max
    return tsdf, pc, timing


def acquire_tsdfs(meshes, n, N=None, resolution=40, size=0.3, device=None, noise=None):
    """The (B, R, R, R) device grid of B scene meshes, each seen from the top-view circle: one render launch, one fusion launch.
    noise: a `giga_amd.noise.DepthNoise` applied in one launch in between; view k of mesh b has the image id (b << 16) | k."""
    intrinsic = sim_intrinsic()
    extrinsics = acquire_extrinsics(n, N, size)
    depth, offs = render_depth_batch(meshes, intrinsic, [extrinsics] * len(meshes), SIM_NEAR, SIM_FAR, 0.0, device)
    if noise is not None and len(depth):
        if n >= 1 << 16:
            raise ValueError("65 536 or more views per scene have no image ids")
        depth = noise.apply(depth, [(b << 16) | k for b in range(len(meshes)) for k in range(n)])
    batches = [depth[offs[b]:offs[b + 1]] for b in range(len(meshes))]
    return perception.fuse_scenes(size, resolution, batches, intrinsic, [extrinsics] * len(meshes), depth.device)[2]


def pose_list(extrinsic):
    """4x4 -> [qx, qy, qz, qw, x, y, z], the reference's Transform.to_list (utils/transform.py)."""
    from scipy.spatial.transform import Rotation
    m = perception.extrinsic_matrix(extrinsic)
    return np.r_[Rotation.from_matrix(m[:3, :3]).as_quat(), m[:3, 3]]


def write_raw_scenes(raw_root, scene_ids, meshes, n, N=None, size=0.3, batch=32, device=None, extrinsics_dtype=np.float32):
    """The raw files scripts/generate_data_parallel.py leaves for construct_dataset: <raw_root>/setup.json (size and intrinsic;
    other keys of an existing file are kept) and <raw_root>/scenes/<id>.npz with depth_imgs (n, H, W) float32 and extrinsics
    (n, 7) float32 [qx, qy, qz, qw, x, y, z] (io.write_sensor_data), rendered from the top-view circle, `batch` scenes per launch.
    extrinsics_dtype=np.float64 stores the poses unrounded: the images were rendered from the float64 cameras, and a float32 pose
    moves the camera `construct_dataset` fuses them with by up to 2e-8, which shows in the last bits of the fused grid."""
    if len(scene_ids) != len(meshes):
        raise ValueError("one scene id per mesh")
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    raw_root = Path(raw_root)
    (raw_root / "scenes").mkdir(parents=True, exist_ok=True)
    intrinsic = sim_intrinsic()
    setup = {}
    if (raw_root / "setup.json").exists():
        with (raw_root / "setup.json").open("r") as f:
            setup = json.load(f)
    setup.update({"size": size, "intrinsic": intrinsic.to_dict()})
    with (raw_root / "setup.json").open("w") as f:
        json.dump(setup, f)
    extrinsics = acquire_extrinsics(n, N, size)
    poses = np.stack([pose_list(e) for e in extrinsics]).astype(extrinsics_dtype) if n else np.zeros((0, 7), extrinsics_dtype)
    for at in range(0, len(meshes), int(batch)):
        chunk = meshes[at:at + int(batch)]
        depth, offs = render_depth_batch(chunk, intrinsic, [extrinsics] * len(chunk), SIM_NEAR, SIM_FAR, 0.0, device)
        depth = depth.cpu().numpy()
        for b, sid in enumerate(scene_ids[at:at + int(batch)]):
            np.savez_compressed(raw_root / "scenes" / (str(sid) + ".npz"), depth_imgs=depth[offs[b]:offs[b + 1]], extrinsics=poses)
    return list(scene_ids)


# ------------------------------------------------------------------------------------------------ occupancy labels
def mesh_bounds(mesh_list):
    """(2, 3) float64: the axis-aligned bounds of all vertices (trimesh's scene.bounds)."""
    vs = [ragged.mesh_parts(m)[0] for m in mesh_list]
    vs = [(v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)).reshape(-1, 3).astype(np.float64) for v in vs]
    v = np.concatenate(vs)
    return np.stack([v.min(axis=0), v.max(axis=0)])


def sample_iou_points(mesh_list, bounds, num_point, padding=0.02, uniform=False, size=0.3, generator=None, device=None):
    """utils/implicit.py:78-90: num_point uniform points in [-padding, size + padding]^3 (uniform) or in the bounds grown by the
    padding, and whether each lies inside ANY mesh of the list.  Returns (points (n, 3) float32, occ (n,) bool) on the device.
    The points come from torch.rand on the device (`generator`: a device generator); the affine map is evaluated in float64 as
    numpy does and rounded to float32 once, and the containment is tested on those float32 points, so the labels belong to the
    returned points.  One ragged giga_mesh_contains launch with one scene per mesh."""
    if generator is not None and device is None:
        device = generator.device
    dev = _capi.hip_device(*ragged.mesh_arrays(mesh_list), device=device, what="occupancy labels are computed on a HIP device")
    points = torch.rand((int(num_point), 3), dtype=torch.float32, device=dev, generator=generator)
    p = points.double()
    if uniform:
        p = p * (size + 2 * padding) - padding
    else:
        b = torch.as_tensor(np.asarray(bounds, np.float64).reshape(2, 3), device=dev)
        p = p * (b[1] + 2 * padding - b[0]) + b[0] - padding
    points = p.float()
    occ = torch.zeros(int(num_point), dtype=torch.bool, device=dev)
    live = [m for m in mesh_list if len(ragged.mesh_parts(m)[1])]
    if live and num_point:
        inside, po = mesh_contains_batch(live, [points] * len(live))
        occ = inside.reshape(len(live), int(num_point)).any(dim=0)
    return points, occ


def save_occ(raw_root, scene_id, mesh_list, num_point_per_file, num_file, uniform=False, generator=None, device=None):
    """scripts/save_occ_data_parallel.py:16-24 for one scene: <raw_root>/occ/<scene_id>/%04d.npz, each with points
    (num_point_per_file, 3) float16 and occ (num_point_per_file,) bool: the files giga_amd.dataset reads.  Like the reference it
    refuses to write into an existing directory."""
    points, occ = sample_iou_points(mesh_list, mesh_bounds(mesh_list), num_point_per_file * num_file, uniform=uniform,
                                    generator=generator, device=device)
    points = points.cpu().numpy().astype(np.float16).reshape(num_file, num_point_per_file, 3)
    occ = occ.cpu().numpy().reshape(num_file, num_point_per_file)
    save_root = os.path.join(str(raw_root), "occ", str(scene_id))
    os.makedirs(save_root)
    for i in range(num_file):
        np.savez(os.path.join(save_root, "%04d.npz" % i), points=points[i], occ=occ[i])
    return save_root
