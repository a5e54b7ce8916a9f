"""Affordance visualisation on the device: the scene mesh coloured by grasp quality, with the selected grippers drawn in.

`affordance_faces` / `affordance_visual` are `vgn.utils.visual.affordance_visual` (reference src/vgn/utils/visual.py:22-98) through
`giga_affordance_points` and `giga_affordance_faces` (csrc/giga_affordance.hip; the arithmetic is spelled out in
include/giga_hip.h): the voxels whose processed quality exceeds `th` become points, every face of the scene mesh aggregates the
quality of the points near its centre, and matplotlib's 'Reds' map turns that into a face colour.  `grasp2mesh` is the gripper
glyph of visual.py:101-142, built on the host.  `ColoredMesh` and `Scene` stand in for `trimesh.Trimesh` and `trimesh.Scene`
(trimesh is an optional dependency) and write `.ply` and `.obj` files themselves.  There is no CPU path for the affordance: CPU
tensors raise `GigaHipError`.

Colours: the 256-entry 'Reds' table is rebuilt from its nine ColorBrewer anchors (`REDS_ANCHORS`, linear interpolation at
i / 255), so matplotlib is not needed; a float colour c becomes the byte rint(255 c).  trimesh has a float-to-uint8 rule of its
own for `face_colors`, which could not be compared where this was written: a byte may differ by one from what the reference
stores.  Where the reference returns the mesh uncoloured (no voxel above `th`), every face gets trimesh's default grey
(102, 102, 102, 255) and the affordance is None.

`render_mesh` / `Scene.render` / `Scene.save_image` turn the composed scene into a picture on a headless device (visual.py:147-164,
pyrender there) through `giga_color_render` (giga_amd/render.py), with `get_camera_pose` (the reference's formula), `look_at` and
`extrinsic_from_camera_pose` for the camera and `write_png` (zlib only) for the file.  The shading is flat and two-sided, one
point or directional light plus an ambient term: the project's own model, not pyrender's metallic-roughness one.

Not reproduced: pyrender's shading model, smooth shading, textures, shadows and transparency (the gripper's alpha of 180 is
ignored); NViSII; the matplotlib plotting helpers."""
from dataclasses import dataclass, field
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _capi, ragged

REDS_ANCHORS = ("fff5f0", "fee0d2", "fcbba1", "fc9272", "fb6a4a", "ef3b2c", "cb181d", "a50f15", "67000d")    # ColorBrewer 'Reds', 9 classes
DEFAULT_FACE_COLOR = (102, 102, 102, 255)         # trimesh's colour of a face that was given none
GRIPPER_COLOR = (0, 250, 0, 180)                  # visual.py:104
CYLINDER_SECTIONS = 32


# ------------------------------------------------------------------------------------------------------------- colour map
def reds_table():
    """(256, 4) float64: matplotlib.colormaps['Reds'] as its lookup table, alpha 1."""
    a = np.array([[int(h[i:i + 2], 16) / 255.0 for i in (0, 2, 4)] for h in REDS_ANCHORS])
    x = np.arange(256) / 255.0
    t = np.ones((256, 4))
    for c in range(3):
        t[:, c] = np.interp(x, np.arange(9) / 8.0, a[:, c])
    return t


def reds(x):
    """matplotlib.colormaps['Reds'](x) for float x of any shape -> (..., 4) float64: entry int(256 x), 1.0 and beyond the last
    entry, below 0 the first, NaN (0, 0, 0, 0)."""
    x = np.asarray(x, np.float64)
    bad = np.isnan(x)
    i = np.clip(np.where(bad, 0.0, x) * 256.0, 0.0, 255.0).astype(np.int64)
    out = reds_table()[i]
    out[bad] = 0.0
    return out


def to_uint8(colors):
    return np.rint(255.0 * np.asarray(colors, np.float64)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------ mesh records
@dataclass
class ColoredMesh:
    """vertices (V,3) float32, faces (F,3) int64, face_colors (F,4) uint8 RGBA, all numpy; `ranges` names runs of faces
    (name -> (first, end)); `affordance` is the (F,) float64 device tensor the colours came from, or None."""
    vertices: np.ndarray
    faces: np.ndarray
    face_colors: np.ndarray
    ranges: Dict[str, Tuple[int, int]] = field(default_factory=dict)
    affordance: Optional[torch.Tensor] = None

    def __post_init__(self):
        self.vertices = np.ascontiguousarray(np.asarray(self.vertices, np.float32).reshape(-1, 3))
        self.faces = np.ascontiguousarray(np.asarray(self.faces, np.int64).reshape(-1, 3))
        self.face_colors = np.ascontiguousarray(np.asarray(self.face_colors, np.uint8).reshape(-1, 4))
        if len(self.face_colors) != len(self.faces):
            raise ValueError("one colour per face")

    def to_trimesh(self):
        import trimesh                       # optional: raises ImportError where it is not installed
        return trimesh.Trimesh(self.vertices, self.faces, face_colors=self.face_colors, process=False)

    def export(self, path):
        """binary little-endian .ply with per-face red green blue alpha, or .obj (geometry only, what Logger.log_mesh writes)"""
        path = str(path)
        if path.lower().endswith(".ply"):
            _write_ply(path, self.vertices, self.faces, self.face_colors)
        elif path.lower().endswith(".obj"):
            _write_obj(path, self.vertices, self.faces)
        else:
            raise ValueError(f"export writes .ply or .obj, not {path!r}")
        return path


class Scene(ColoredMesh):
    """Named meshes composed into one (the role of trimesh.Scene in detection_implicit.py:80-82): `add_geometry` appends a mesh
    and records its faces under `node_name` in `ranges`."""

    def __init__(self, mesh=None, node_name="scene"):
        super().__init__(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), np.zeros((0, 4), np.uint8), {}, None)
        if mesh is not None:
            self.add_geometry(mesh, node_name)

    def add_geometry(self, mesh, node_name=None):
        name = node_name if node_name is not None else f"geometry_{len(self.ranges)}"
        if name in self.ranges:
            raise ValueError(f"the scene already holds {name!r}")
        first = len(self.faces)
        self.faces = np.concatenate((self.faces, mesh.faces + len(self.vertices)))
        self.vertices = np.concatenate((self.vertices, mesh.vertices))
        self.face_colors = np.concatenate((self.face_colors, mesh.face_colors))
        self.ranges[name] = (first, len(self.faces))
        if name == "scene":
            self.affordance = mesh.affordance
        return name

    def geometry(self, name):
        a, b = self.ranges[name]
        return self.faces[a:b], self.face_colors[a:b]

    def render(self, camera_pose=None, **kw):
        """`render_mesh` of the composed scene: (H, W, 3) uint8 numpy array.  camera_pose: an OpenGL camera-to-world pose
        (`get_camera_pose`, `look_at`); None is the side-view camera of `render.acquire_extrinsics(sideview=True)`."""
        return render_mesh(self, camera_pose, **kw)

    def save_image(self, path, **kw):
        """`render` written as an 8-bit RGB .png; returns the path"""
        return write_png(path, self.render(**kw))


def _write_ply(path, vertices, faces, colors):
    if len(vertices) >= 2 ** 31:
        raise ValueError("a .ply face indexes at most 2^31 - 1 vertices")
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {len(vertices)}\nproperty float x\nproperty float y\nproperty float z\n"
              f"element face {len(faces)}\nproperty list uchar int vertex_indices\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n")
    rec = np.zeros(len(faces), np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("c", "u1", (4,))]))
    rec["n"] = 3
    rec["v"] = faces
    rec["c"] = colors
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(vertices, "<f4").tobytes())
        f.write(rec.tobytes())


def _write_obj(path, vertices, faces):
    with open(path, "w") as f:
        for v in vertices:
            f.write("v %.9g %.9g %.9g\n" % (v[0], v[1], v[2]))       # nine digits bring a float32 back exactly
        for t in faces + 1:
            f.write("f %d %d %d\n" % (t[0], t[1], t[2]))


# ---------------------------------------------------------------------------------------------------------------- affordance
class _Affordance:
    """One giga_affordance_points + giga_affordance_faces pair in flight: `launch` enqueues both on the current stream without
    synchronising, `finish` reads the point counts (the only device-to-host traffic) and splits the packed results."""

    def __init__(self, qual_vol, rot_vol, meshes, size=0.3, th=0.5, temp=150, rad=0.02, finger_depth=0.05, finger_offset=0.5,
                 move_center=True, aggregation="max", dense=False):
        if aggregation not in _capi.AFFORDANCE:
            raise ValueError(f"aggregation is 'max', 'softmax' or 'mean', not {aggregation!r}")
        if not (torch.is_tensor(qual_vol) and torch.is_tensor(rot_vol)):
            raise _capi.GigaHipError("affordance_faces takes the volumes as device tensors; there is no CPU fallback")
        dev = _capi.device_of(qual_vol, rot_vol, *[x for x in ragged.mesh_arrays(meshes) if torch.is_tensor(x)])
        R = int(qual_vol.shape[-1])
        if qual_vol.dim() not in (3, 4) or tuple(qual_vol.shape[-3:]) != (R, R, R):
            raise ValueError(f"expected a (B,R,R,R) or (R,R,R) quality volume, got {tuple(qual_vol.shape)}")
        B = 1 if qual_vol.dim() == 3 else int(qual_vol.shape[0])
        V = R * R * R
        if rot_vol.numel() != B * V * 4:
            raise ValueError(f"expected {B} x {V} quaternions, got a tensor of shape {tuple(rot_vol.shape)}")
        if len(meshes) != B:
            raise ValueError(f"{B} volumes and {len(meshes)} meshes")
        self.B, self.R, self.dev = B, R, dev
        self.qual = qual_vol.detach().reshape(B, V).float().contiguous()
        self.rot = rot_vol.detach().reshape(B, V, 4).float().contiguous()
        self.v, self.vo, self.f, self.fo = ragged.pack_meshes(meshes, dev)
        self.prm = _capi.AffordanceParams(float(size), float(th), float(temp), float(rad), float(finger_depth), float(finger_offset),
                                          int(bool(move_center)), _capi.AFFORDANCE[aggregation] | (_capi.AFFORDANCE_DENSE if dense else 0))
        F = int(self.fo[-1])
        self.points = torch.empty((B, V, 4), dtype=torch.float64, device=dev)
        self.counts = torch.zeros(B, dtype=torch.int32, device=dev)
        self.affordance = torch.empty(F, dtype=torch.float64, device=dev)
        self.rgba = torch.empty((F, 4), dtype=torch.uint8, device=dev)
        self.ws = _capi.workspace("giga_affordance", dev, B, R, F)

    def launch(self):
        B, R, ws = self.B, self.R, self.ws
        _capi.call("giga_affordance_points", self.dev, self.qual, self.rot, B, R, self.prm, self.points, self.counts, ws, ws.numel())
        _capi.call("giga_affordance_faces", self.dev, self.v, self.vo, self.f, self.fo, self.points, self.counts, B, R, self.prm,
                   self.affordance, self.rgba, ws, ws.numel())
        return self

    def finish(self):
        """[(affordance (F,) float64 device tensor or None, colours (F,4) uint8 device tensor)] per scene"""
        self.n_points = self.counts.cpu().numpy().astype(np.int64)
        fo = self.fo
        return [(self.affordance[fo[b]:fo[b + 1]] if self.n_points[b] > 0 else None, self.rgba[fo[b]:fo[b + 1]])
                for b in range(self.B)]


def affordance_points(qual_vol, rot_vol, size=0.3, th=0.5, finger_depth=0.05, finger_offset=0.5, move_center=True):
    """The point cloud the affordance is aggregated from: per scene a (P, 4) float64 device tensor (x, y, z, q) of the voxels with
    q > float32(th), in voxel order (positions on np.linspace(0, size, R)^3, moved by the gripper's z axis when move_center)."""
    B = 1 if qual_vol.dim() == 3 else int(qual_vol.shape[0])
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    a = _Affordance(qual_vol, rot_vol, [empty] * B, size=size, th=th, finger_depth=finger_depth, finger_offset=finger_offset,
                    move_center=move_center).launch()
    a.finish()
    out = [a.points[b, :int(a.n_points[b])] for b in range(B)]
    return out if qual_vol.dim() == 4 else out[0]


def affordance_faces(qual_vol, rot_vol, meshes, size=0.3, th=0.5, temp=150, rad=0.02, finger_depth=0.05, finger_offset=0.5,
                     move_center=True, aggregation="max", dense=False):
    """Affordance and colour of every face of B scene meshes.

    qual_vol (B,R,R,R) | (R,R,R): the quality volume after process and bound (`grasp_select(..., return_volume=True)`); rot_vol
    (B,R^3,4) | (R,R,R,4): the quaternions (xyzw); both device tensors.  meshes: a list of B meshes, or one mesh for one scene;
    a mesh is a (vertices, faces) pair of numpy arrays or device tensors, or an object with these attributes.  The remaining
    arguments are those of the reference's affordance_visual.  dense=True keeps the faces x points form where 'max' would walk
    the cell grid (the results are the same bytes).

    Returns, per scene, (affordance, colours): (F,) float64, or None when no voxel exceeds th, and (F,4) uint8 RGBA, both on the
    device -- a list of such pairs for a list of meshes, one pair for one mesh.  The only device-to-host traffic is the point
    counts."""
    single = not isinstance(meshes, list)
    out = _Affordance(qual_vol, rot_vol, [meshes] if single else meshes, size, th, temp, rad, finger_depth, finger_offset, move_center,
                      aggregation, dense).launch().finish()
    return out[0] if single else out


def _colored(mesh, affordance, rgba):
    v, f = ragged.mesh_parts(mesh)
    v, f = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (v, f))
    m = ColoredMesh(v, f, rgba.cpu().numpy(), affordance=affordance)
    m.ranges["scene"] = (0, len(m.faces))
    return m


def affordance_visual(qual_vol, rot_vol, scene_mesh, size=0.3, resolution=40, **aff_kwargs):
    """The reference's affordance_visual for one scene, with its argument order: a `ColoredMesh` of scene_mesh whose faces carry
    the affordance colours (and the affordance itself, a device tensor or None, as `.affordance`)."""
    if int(qual_vol.shape[-1]) != int(resolution):
        raise ValueError(f"a volume of {int(qual_vol.shape[-1])}^3 voxels with resolution={resolution}")
    aff, rgba = affordance_faces(qual_vol.reshape((resolution,) * 3), rot_vol, scene_mesh, size=size, **aff_kwargs)
    return _colored(scene_mesh, aff, rgba)


# ------------------------------------------------------------------------------------------------------------------ gripper
def _quat_matrix(q):
    """xyzw quaternion -> 3x3 rotation matrix in float64 (normalised first, as scipy's Rotation does)"""
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(np.asarray(q, np.float64))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def cylinder(radius, height, sections=CYLINDER_SECTIONS):
    """A capped cylinder about the z axis, centred on the origin: (2 sections + 2, 3) float64 vertices (the two cap centres, the
    bottom rim, the top rim) and (4 sections, 3) int64 faces wound so that the normals point outwards."""
    n = sections
    a = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack((radius * np.cos(a), radius * np.sin(a)), -1)
    v = np.zeros((2 * n + 2, 3))
    v[0, 2], v[1, 2] = -height / 2.0, height / 2.0
    v[2:n + 2, :2], v[2:n + 2, 2] = rim, -height / 2.0
    v[n + 2:, :2], v[n + 2:, 2] = rim, height / 2.0
    i = np.arange(n)
    j = (i + 1) % n
    b0, b1, t0, t1 = 2 + i, 2 + j, n + 2 + i, n + 2 + j
    zero, one = np.zeros(n, np.int64), np.ones(n, np.int64)
    f = np.concatenate((np.stack((zero, b1, b0), -1), np.stack((one, t0, t1), -1),
                        np.stack((b0, b1, t1), -1), np.stack((b0, t1, t0), -1)))
    return v, f.astype(np.int64)


def gripper_parts(width, finger_depth=0.05):
    """The four cylinders of visual.py:101-142 in the gripper's frame: [(name, local 4x4 transform, radius, height)]"""
    w, d = float(width), float(finger_depth)

    def pose(rot, t):
        m = np.eye(4)
        m[:3, :3], m[:3, 3] = rot, t
        return m
    quarter_x = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0.0, 1.0, 0.0]])      # pi / 2 about x, exactly
    r = 0.1 * d
    return [("left_finger", pose(np.eye(3), [0.0, -w / 2, d / 2]), r, d),
            ("right_finger", pose(np.eye(3), [0.0, w / 2, d / 2]), r, d),
            ("wrist", pose(np.eye(3), [0.0, 0.0, -d / 4]), r, d / 2),
            ("palm", pose(quarter_x, [0.0, 0.0, 0.0]), r, w)]


def gripper_geometry(grasp, finger_depth=0.05):
    """(vertices (264,3) float64, faces (512,3) int64) of the gripper glyph of `grasp` in the task frame"""
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = _quat_matrix(grasp["rotation"]), np.asarray(grasp["translation"], np.float64)
    verts, faces, base = [], [], 0
    for _, local, radius, height in gripper_parts(grasp["width"], finger_depth):
        v, f = cylinder(radius, height)
        m = T @ local                              # grasp.pose * Transform(...)
        verts.append(v @ m[:3, :3].T + m[:3, 3])
        faces.append(f + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces)


def grasp2mesh(grasp, score=None, finger_depth=0.05):
    """The gripper glyph of visual.py:101-142 as a `ColoredMesh`: two fingers, wrist and palm, four capped cylinders of radius
    0.1 finger_depth posed by the grasp, every face (0, 250, 0, 180).  grasp: the dict this package's planner returns
    (rotation xyzw, translation, width); score is accepted and unused, as in the reference.  Built on the host in float64.
    The tessellation is this package's own (32 sections, capped: 66 vertices and 128 outward-wound faces per cylinder);
    vertex-for-vertex equality with trimesh.creation.cylinder is not claimed."""
    v, f = gripper_geometry(grasp, finger_depth)
    return ColoredMesh(v, f, np.tile(np.array(GRIPPER_COLOR, np.uint8), (len(f), 1)))


# ---------------------------------------------------------------------------------------------------------------- rendering
def get_camera_pose(radius, center=(0.0, 0.0, 0.0), ax=0, ay=0, az=0):
    """visual.py:147-155: the OpenGL camera-to-world pose (the camera looks down its -z axis, y up) at distance `radius` from
    `center`: rotation = Rotation.from_euler('xyz', (ax, ay, az)) = Rz(az) Ry(ay) Rx(ax), translation = rotation (0, 0, radius)
    + center.  4x4 float64."""
    (cx, sx), (cy, sy), (cz, sz) = ((np.cos(a), np.sin(a)) for a in (float(ax), float(ay), float(az)))
    rx = np.array([[1.0, 0.0, 0.0], [0.0, cx, -sx], [0.0, sx, cx]])
    ry = np.array([[cy, 0.0, sy], [0.0, 1.0, 0.0], [-sy, 0.0, cy]])
    rz = np.array([[cz, -sz, 0.0], [sz, cz, 0.0], [0.0, 0.0, 1.0]])
    pose = np.eye(4)
    pose[:3, :3] = rz @ ry @ rx
    pose[:3, 3] = pose[:3, :3] @ np.array([0.0, 0.0, float(radius)]) + np.asarray(center, np.float64)
    return pose


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """The OpenGL camera-to-world pose of a camera at `eye` that looks at `target` with `up` upwards in the image."""
    eye, target, up = (np.asarray(x, np.float64).reshape(3) for x in (eye, target, up))
    z = eye - target
    z = z / np.linalg.norm(z)
    x = np.cross(up, z)
    if not np.linalg.norm(x) > 0:
        raise ValueError("up is parallel to the viewing direction")
    x = x / np.linalg.norm(x)
    pose = np.eye(4)
    pose[:3, 0], pose[:3, 1], pose[:3, 2], pose[:3, 3] = x, np.cross(z, x), z, eye
    return pose


def extrinsic_from_camera_pose(pose):
    """OpenGL camera-to-world pose -> this package's extrinsic (world-to-camera, z forward, y down): diag(1, -1, -1, 1) pose^-1,
    the inverse taken as that of a rigid transform."""
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    inv = np.eye(4)
    inv[:3, :3] = pose[:3, :3].T
    inv[:3, 3] = -pose[:3, :3].T @ pose[:3, 3]
    return np.diag([1.0, -1.0, -1.0, 1.0]) @ inv


def render_mesh(mesh, camera_pose=None, light_pose=None, intrinsic=None, ambient=0.3, background=(255, 255, 255, 255), near=None,
                far=None, pixel_offset=0.0, supersample=1, device=None):
    """visual.py:157-164 without pyrender: a `ColoredMesh` / `Scene` seen from the OpenGL camera-to-world pose `camera_pose`
    (None: the side view of `render.acquire_extrinsics`), lit by a point light at the origin of `light_pose` (a camera-to-world
    style 4x4; None: a headlight at the camera).  intrinsic: a `perception.CameraIntrinsic`, default `render.sim_intrinsic()`;
    near / far default to the simulated camera's 0.1 / 2.0.  Returns an (H, W, 3) uint8 numpy array.  Flat, two-sided shading of
    the face colours through `giga_color_render`: the project's own model (include/giga_hip.h), not pyrender's
    metallic-roughness one; the faces' alpha is not used."""
    from . import render
    intrinsic = render.sim_intrinsic() if intrinsic is None else intrinsic
    ext = render.acquire_extrinsics(1, sideview=True)[0] if camera_pose is None else extrinsic_from_camera_pose(camera_pose)
    light = None
    if light_pose is not None:
        at = ext @ np.r_[np.asarray(light_pose, np.float64).reshape(4, 4)[:3, 3], 1.0]
        light = (at[0], at[1], at[2], 1.0)
    rgba = render.render_color(mesh.vertices, mesh.faces, mesh.face_colors, intrinsic, [ext], lights=light, ambient=ambient,
                               background=background, near=render.SIM_NEAR if near is None else near,
                               far=render.SIM_FAR if far is None else far, pixel_offset=pixel_offset, supersample=supersample,
                               device=device)
    return np.ascontiguousarray(rgba[0, :, :, :3].cpu().numpy())


def write_png(path, image):
    """(H, W, 3) or (H, W, 4) uint8 array (numpy or tensor) -> an 8-bit RGB / RGBA .png without interlace, every row with filter
    0, through the standard library's zlib.  Returns the path."""
    import struct
    import zlib
    a = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("write_png takes an (H, W, 3) or (H, W, 4) uint8 image")
    H, W, C = a.shape
    rows = np.zeros((H, 1 + W * C), np.uint8)          # filter type 0 in front of every row
    rows[:, 1:] = a.reshape(H, W * C)

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xffffffff)
    with open(str(path), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + chunk(b"IEND", b""))
    return str(path)
