"""Input side of the hot path: depth images to the network's grid on the device.

`TSDFVolume` / `create_tsdf` / `create_tsdfs` fuse depth images with camera poses into a truncated signed distance volume
(`giga_tsdf_integrate`), export the (1, R, R, R) grid the encoder consumes in the same pass and extract the zero-crossing
point cloud (`giga_tsdf_cloud_count` / `_emit`): the counterpart of `vgn.perception` (reference src/vgn/perception.py:10-137),
which hands these steps to Open3D.  The arithmetic restates Open3D's UniformTSDFVolume (NoColor) operation by operation
(include/giga_hip.h); `construct_dataset` is the loop of scripts/construct_dataset_parallel.py on top of it, depth noise
(`giga_amd.noise.DepthNoise`, its `noise=` argument) included.

Dense export of a sparse voxel list that Open3D has already produced on the host:

Counterpart of `vgn.perception.TSDFVolume.get_grid` (reference src/vgn/perception.py:107-115), which fills a
(1, R, R, R) float32 grid from Open3D's sparse voxel list with a Python loop over the voxels (the reference notes
"very slow (~35 ms / 50 ms of the whole pipeline)").  Here the sparse list is uploaded once (16 B per voxel) and a HIP
kernel scatters it into the dense grid the encoder consumes, for any number of scenes per call (`giga_tsdf_scatter`)."""
import json
from math import cos, sin
from pathlib import Path

import numpy as np
import torch

from . import _capi


def voxel_arrays(voxels):
    """(index (n,3) int32, value (n,) float32) from an iterable of Open3D-style voxels (`.grid_index`, `.color`): the two
    attributes the reference loop reads (perception.py:112-114)."""
    idx = np.asarray([v.grid_index for v in voxels], dtype=np.int32).reshape(-1, 3)
    val = np.asarray([v.color[0] for v in voxels], dtype=np.float32).reshape(-1)
    return idx, val


def dense_grids(scenes, resolution=40, device=None):
    """scenes: list of (index (n_b,3) int, value (n_b,) float) per scene (numpy arrays or tensors).
    Returns a (B, R, R, R) float32 device tensor: 0 where unobserved, else the value of the last listed voxel of the cell."""
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise _capi.GigaHipError("dense_grids runs on a HIP device; use the reference's get_grid on the CPU")
    R, B = int(resolution), len(scenes)
    idx_l, val_l, offs = [], [], [0]
    for idx, val in scenes:
        idx = torch.as_tensor(idx).reshape(-1, 3)
        val = torch.as_tensor(val).reshape(-1)
        if idx.shape[0] != val.shape[0]:
            raise ValueError("one value per voxel index")
        if not idx.is_cuda and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= R):
            raise IndexError(f"voxel grid_index outside [0, {R})")       # numpy raises (or wraps negatives) in the reference loop
        idx_l.append(idx.to(torch.int32)); val_l.append(val.to(torch.float32))
        offs.append(offs[-1] + idx.shape[0])
    grid = torch.empty((B, R, R, R), dtype=torch.float32, device=device)
    if B == 0:
        return grid
    n = offs[-1]
    index = torch.cat(idx_l).to(device).contiguous() if n else None
    value = torch.cat(val_l).to(device).contiguous() if n else None
    offsets = torch.tensor(offs, dtype=torch.int32).to(device)
    ws = _capi.workspace("giga_tsdf_scatter", device, B, R)
    _capi.call("giga_tsdf_scatter", device, index, value, offsets, B, R, n, grid, ws, ws.numel())
    return grid


def dense_grid(voxel_index, voxel_value, resolution=40, device=None):
    """One scene, in the reference's return shape (1, R, R, R) (perception.py:109)."""
    return dense_grids([(voxel_index, voxel_value)], resolution, device)


# ------------------------------------------------------------------------------------------------ cameras
class CameraIntrinsic(object):
    """Intrinsic parameters of a pinhole camera model (perception.py:10-60): width, height, K."""

    def __init__(self, width, height, fx, fy, cx, cy):
        self.width = width
        self.height = height
        self.K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])

    @property
    def fx(self):
        return self.K[0, 0]

    @property
    def fy(self):
        return self.K[1, 1]

    @property
    def cx(self):
        return self.K[0, 2]

    @property
    def cy(self):
        return self.K[1, 2]

    def to_dict(self):
        return {"width": self.width, "height": self.height, "K": self.K.flatten().tolist()}

    @classmethod
    def from_dict(cls, data):
        K = data["K"]
        return cls(width=data["width"], height=data["height"], fx=K[0], fy=K[4], cx=K[2], cy=K[5])


def extrinsic_matrix(extrinsic):
    """4x4 float64 matrix (task -> camera) of an extrinsic given as a 4x4 matrix, as the 7-list [qx, qy, qz, qw, x, y, z] that
    the reference's Transform.to_list writes (utils/transform.py), or as any object with as_matrix()."""
    if hasattr(extrinsic, "as_matrix"):
        m = np.asarray(extrinsic.as_matrix(), np.float64)
    else:
        m = np.asarray(extrinsic, np.float64)
        if m.shape == (7,):
            from scipy.spatial.transform import Rotation
            pose = m
            m = np.eye(4)
            m[:3, :3] = Rotation.from_quat(pose[:4]).as_matrix()          # Transform.from_list -> as_matrix
            m[:3, 3] = pose[4:]
    if m.shape != (4, 4):
        raise ValueError("an extrinsic is a 4x4 matrix, a 7-list [qx, qy, qz, qw, x, y, z] or an object with as_matrix()")
    return np.ascontiguousarray(m)


def camera_on_sphere(origin, radius, theta, phi):
    """perception.py:129-137: the extrinsic (4x4, task -> camera) of a camera on a sphere about `origin` (any extrinsic form)
    that looks at it with z up: Transform.look_at(eye, 0, z) * origin.inverse()."""
    eye = np.r_[radius * sin(theta) * cos(phi), radius * sin(theta) * sin(phi), radius * cos(theta)]
    up = np.array([0.0, 0.0, 1.0])               # (breaks when looking straight down, like the reference)
    forward = -eye / np.linalg.norm(eye)
    right = np.cross(forward, up)
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    rot = np.stack((right, -up, forward), 1)     # camera -> reference frame, columns = camera axes
    look = np.eye(4)
    look[:3, :3] = rot.T                         # the inverse of (rot, eye)
    look[:3, 3] = -rot.T @ eye
    o = extrinsic_matrix(origin)
    o_inv = np.eye(4)
    o_inv[:3, :3] = o[:3, :3].T
    o_inv[:3, 3] = -o[:3, :3].T @ o[:3, 3]
    return look @ o_inv


# ------------------------------------------------------------------------------------------------ fusion
DEPTH_SCALE, DEPTH_TRUNC = 1.0, 2.0              # perception.py:89-90
CLOUD_LOWER, CLOUD_UPPER = np.array([0.02, 0.02, 0.055]), np.array([0.28, 0.28, 0.3])      # construct_dataset_parallel.py:31-32
FUSION_DEVICE = "depth fusion runs on a HIP device"


def integrate_batch(tsdf, weight, depth, view_offsets, intrinsic, extrinsics, size, grid=None):
    """One `giga_tsdf_integrate` launch.  tsdf, weight (B, R, R, R) float32 device tensors (updated in place); depth
    (n, H, W) float32 device tensor with the views of all scenes back to back; view_offsets B + 1 ints; extrinsics n
    extrinsics (any form); grid: optional (B, R, R, R) output.  Asynchronous on the current stream."""
    dev = _capi.device_of(tsdf, weight, depth, grid)
    B, R = tsdf.shape[0], tsdf.shape[-1]
    offs = np.ascontiguousarray(view_offsets, np.int32)
    n = int(offs[-1]) if len(offs) else 0
    if len(offs) != B + 1 or depth.shape[0] != n or len(extrinsics) != n:
        raise ValueError("view_offsets has B + 1 entries and counts the depth images and extrinsics")
    for t in (tsdf, weight, grid):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != B * R ** 3):
            raise ValueError("tsdf, weight and grid are contiguous float32 (B, R, R, R) tensors")
    if depth.dtype != torch.float32 or not depth.is_contiguous():
        raise ValueError("depth is a contiguous float32 (n, H, W) tensor")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if (H, W) != (int(intrinsic.height), int(intrinsic.width)):
        raise ValueError(f"depth images are {H}x{W}, the intrinsic says {intrinsic.height}x{intrinsic.width}")
    ext = np.ascontiguousarray(np.stack([extrinsic_matrix(e) for e in extrinsics]).reshape(n, 16)) if n else np.zeros((0, 16))
    cam = np.ascontiguousarray(np.tile(np.array([intrinsic.fx, intrinsic.fy, intrinsic.cx, intrinsic.cy], np.float64), (n, 1)))
    ws = _capi.workspace("giga_tsdf_integrate", dev, B, n)
    _capi.call("giga_tsdf_integrate", dev, depth, offs, ext, cam, B, W, H, float(size), R, 4.0 * (float(size) / R), DEPTH_SCALE,
               DEPTH_TRUNC, tsdf, weight, grid, ws, ws.numel())


def cloud_batch(tsdf, weight, size, capacity=None, normals=False):
    """Zero-crossing points of B volumes: ((n, 3) float32 device tensor, scenes back to back; B + 1 host offsets).  With
    `capacity` the points beyond it are dropped (the offsets still count all of them).  normals=True: (points, normals, offsets),
    the normals an (n, 3) float32 device tensor, one per point (`giga_tsdf_cloud_emit_oriented`; the points are the same bytes)."""
    dev = _capi.device_of(tsdf, weight)
    B, R = tsdf.shape[0], tsdf.shape[-1]
    if B == 0:
        empty = torch.empty((0, 3), device=dev)
        return (empty, torch.empty((0, 3), device=dev), np.zeros(1, np.int64)) if normals else (empty, np.zeros(1, np.int64))
    ws = _capi.workspace("giga_tsdf_cloud", dev, B, R)
    counts = torch.empty(B, dtype=torch.int32, device=dev)
    _capi.call("giga_tsdf_cloud_count", dev, tsdf, weight, B, R, ws, ws.numel(), counts)
    offsets = np.concatenate(([0], np.cumsum(counts.cpu().numpy().astype(np.int64))))
    cap = int(offsets[-1]) if capacity is None else min(int(capacity), int(offsets[-1]))
    points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    if normals:
        nrm = torch.empty((cap, 3), dtype=torch.float32, device=dev)
        _capi.call("giga_tsdf_cloud_emit_oriented", dev, tsdf, weight, B, R, float(size), ws, ws.numel(), points if cap else None,
                   nrm if cap else None, cap, None)
        return points, nrm, offsets
    _capi.call("giga_tsdf_cloud_emit", dev, tsdf, weight, B, R, float(size), ws, ws.numel(), points if cap else None, cap, None)
    return points, offsets


class TSDFVolume(object):
    """Integration of multiple depth images using a TSDF (perception.py:63-118), state and grid on the device."""

    def __init__(self, size, resolution, device=None):
        self.size = size
        self.resolution = resolution
        self.voxel_size = self.size / self.resolution
        self.sdf_trunc = 4 * self.voxel_size
        self.device = _capi.hip_device(device=device, what=FUSION_DEVICE)
        R = int(resolution)
        if not 2 <= R <= _capi.TSDF_MAX_R:
            raise ValueError(f"resolution outside 2 .. {_capi.TSDF_MAX_R}")
        self._tsdf = torch.zeros((1, R, R, R), dtype=torch.float32, device=self.device)
        self._weight = torch.zeros_like(self._tsdf)
        self._grid = torch.zeros_like(self._tsdf)

    def integrate(self, depth_img, intrinsic, extrinsic):
        """depth_img (H, W) array or tensor; extrinsic: the transform from the TSDF to camera coordinates, T_eye_task."""
        self.integrate_views(torch.as_tensor(depth_img)[None], intrinsic, [extrinsic])

    def integrate_views(self, depth_imgs, intrinsic, extrinsics):
        """Several views (n, H, W) in one launch; equal to n integrate calls in that order."""
        depth = torch.as_tensor(depth_imgs).to(self.device, torch.float32).contiguous()
        integrate_batch(self._tsdf, self._weight, depth, [0, depth.shape[0]], intrinsic, list(extrinsics), self.size, self._grid)

    def grid(self):
        """The network input (1, R, R, R) as a device tensor (no copy to the host); valid until the next integrate."""
        return self._grid

    def get_grid(self):
        return self._grid.cpu().numpy()

    def state(self):
        """(tsdf, weight): the (1, R, R, R) float32 device tensors the volume integrates into."""
        return self._tsdf, self._weight

    def get_cloud(self, normals=False):
        """(n, 3) float32 device tensor: the zero crossings of extract_point_cloud.  normals=True: (points, normals), the
        normals of extract_point_cloud as a second (n, 3) float32 device tensor."""
        out = cloud_batch(self._tsdf, self._weight, self.size, normals=normals)
        return out[:2] if normals else out[0]


def create_tsdf(size, resolution, depth_imgs, intrinsic, extrinsics, device=None):
    """perception.py:121-126; the views are fused in one launch."""
    tsdf = TSDFVolume(size, resolution, device)
    if len(depth_imgs):
        tsdf.integrate_views(depth_imgs, intrinsic, extrinsics)
    return tsdf


def fuse_scenes(size, resolution, depth_batches, intrinsic, extrinsics_batches, device=None):
    """B scenes with ragged view counts in one launch: depth_batches[b] (V_b, H, W), extrinsics_batches[b] V_b extrinsics.
    Returns (tsdf, weight, grid), each a (B, R, R, R) float32 device tensor."""
    device = _capi.hip_device(device=device, what=FUSION_DEVICE)
    B, R = len(depth_batches), int(resolution)
    if len(extrinsics_batches) != B:
        raise ValueError("one list of extrinsics per scene")
    if not 2 <= R <= _capi.TSDF_MAX_R:
        raise ValueError(f"resolution outside 2 .. {_capi.TSDF_MAX_R}")
    tsdf = torch.zeros((B, R, R, R), dtype=torch.float32, device=device)
    weight, grid = torch.zeros_like(tsdf), torch.zeros_like(tsdf)
    if B == 0:
        return tsdf, weight, grid
    H, W = int(intrinsic.height), int(intrinsic.width)
    imgs = [torch.as_tensor(d).to(torch.float32).reshape(-1, H, W) for d in depth_batches]
    offs = np.concatenate(([0], np.cumsum([len(d) for d in imgs])))
    depth = torch.cat(imgs).to(device).contiguous()
    ext = [e for batch in extrinsics_batches for e in batch]
    integrate_batch(tsdf, weight, depth, offs, intrinsic, ext, size, grid)
    return tsdf, weight, grid


def create_tsdfs(size, resolution, depth_batches, intrinsic, extrinsics_batches, device=None):
    """The (B, R, R, R) device grid of B scenes (ragged view counts) fused in one launch."""
    return fuse_scenes(size, resolution, depth_batches, intrinsic, extrinsics_batches, device)[2]


def _fuse_to_host(size, resolution, depth_batches, intrinsic, extrinsics_batches, device=None):
    """(grids (B, R, R, R) numpy, list of B (n_b, 3) numpy clouds): the device part of construct_dataset."""
    tsdf, weight, grid = fuse_scenes(size, resolution, depth_batches, intrinsic, extrinsics_batches, device)
    points, offsets = cloud_batch(tsdf, weight, size)
    points = points.cpu().numpy()
    return grid.cpu().numpy(), [points[offsets[b]:offsets[b + 1]] for b in range(len(depth_batches))]


def _noise_scenes(noise, depth_batches, image_ids, device=None):
    """noise.apply on the images of several scenes in one launch: depth_batches[b] (V_b, H, W), image_ids one id per image, scenes
    back to back.  Returns the noised (V_b, H, W) float32 device tensors, one per scene."""
    device = _capi.hip_device(device=device, what=FUSION_DEVICE)
    imgs = [torch.as_tensor(d).to(torch.float32) for d in depth_batches]
    out = noise.apply(torch.cat(imgs).to(device), image_ids)
    return list(torch.split(out, [len(d) for d in imgs]))


def construct_dataset(raw_root, dataset_root, single_view=False, batch=32, add_noise="", resolution=40, device=None, noise=None):
    """scripts/construct_dataset_parallel.py: every <raw_root>/scenes/<id>.npz (depth_imgs, extrinsics) becomes
    <dataset_root>/scenes/<id>.npz (grid (1, R, R, R), the layout giga_amd.dataset.read_voxel_grid reads) and
    <dataset_root>/point_clouds/<id>.npz (pc, the cloud cropped to the reference's box); `batch` scenes are fused per launch.
    noise: a `giga_amd.noise.DepthNoise` applied on the device to every depth image that is fused (with single_view: the one
    view that is used), as the reference's --add-noise does (construct_dataset_parallel.py:21); None leaves the images as they
    are.  Image `view` of the scene with ordinal s in the sorted file list has the id (s << 16) | view, so a scene's noise does
    not depend on `batch` (scenes with 65 536 views or more are rejected).  The reference's string flag `add_noise` still
    raises: it draws from numpy's global generator, and a string carries no seed.
    Returns the scene ids in the order they were written."""
    if add_noise:
        raise NotImplementedError("add_noise: the reference's flag draws from numpy's global generator and carries no seed; pass "
                                  "noise=giga_amd.noise.DepthNoise(kind, seed) instead")
    if noise is not None and not callable(getattr(noise, "apply", None)):
        raise TypeError("noise is a giga_amd.noise.DepthNoise (or None)")
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    raw_root, dataset_root = Path(raw_root), Path(dataset_root)
    with (raw_root / "setup.json").open("r") as f:
        setup = json.load(f)
    size, intrinsic = setup["size"], CameraIntrinsic.from_dict(setup["intrinsic"])
    files = sorted(f for f in (raw_root / "scenes").iterdir() if f.suffix == ".npz")
    (dataset_root / "scenes").mkdir(parents=True)              # like the reference: refuses to write into an existing dataset
    (dataset_root / "point_clouds").mkdir(parents=True)
    done = []
    for at in range(0, len(files), int(batch)):
        chunk = files[at:at + int(batch)]
        depth, ext = [], []
        for f in chunk:
            with np.load(f) as data:
                d, e = data["depth_imgs"], data["extrinsics"]
            depth.append(d[:1] if single_view else d)
            ext.append(e[:1] if single_view else e)
        if noise is not None:
            if any(len(d) >= 1 << 16 for d in depth):
                raise ValueError("a scene with 65 536 or more views has no image ids")
            ids = [((at + k) << 16) | v for k, d in enumerate(depth) for v in range(len(d))]
            depth = _noise_scenes(noise, depth, ids, device)
        grids, clouds = _fuse_to_host(size, resolution, depth, intrinsic, ext, device)
        for f, g, pc in zip(chunk, grids, clouds):
            np.savez_compressed(dataset_root / "scenes" / (f.stem + ".npz"), grid=g[None])
            # o3d's AxisAlignedBoundingBox crop keeps min <= p <= max
            keep = np.all((pc >= CLOUD_LOWER) & (pc <= CLOUD_UPPER), axis=1)
            np.savez_compressed(dataset_root / "point_clouds" / (f.stem + ".npz"), pc=pc[keep].astype(np.float64))
            done.append(f.stem)
    return done
