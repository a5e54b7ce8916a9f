"""CPU tests of the affordance visualisation: the numpy restatement of tests/affordance_emu.py against its own scalar-order form,
the 'Reds' table (package, library and restatement against each other, and against matplotlib where it is installed), the gripper
glyph, the .ply / .obj writers, the argument validation of giga_affordance_points / giga_affordance_faces without a device and the
planner's host logic."""
import ctypes
import os

import numpy as np
import pytest

import affordance_emu as aemu
import render_emu as remu
from giga_amd import _capi, visual
from giga_amd.detection import VGNImplicit

F32 = np.float32


def volumes(seed, R):
    rng = np.random.default_rng(seed)
    qual = rng.random((R, R, R), dtype=F32)
    rot = rng.standard_normal((R, R, R, 4)).astype(F32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    return qual, rot


# ------------------------------------------------------------------------------------------- the restatement against itself
@pytest.mark.parametrize("move_center", [True, False])
def test_vectorised_restatement_equals_the_scalar_order_form(move_center):
    qual, rot = volumes(3, 8)
    v, f = remu.icosphere((0.15, 0.15, 0.1), 0.08, 2)
    assert len(f) == 320
    pts = aemu.points(qual, rot, move_center=move_center)
    assert 200 < len(pts) < 320 and pts.dtype == np.float64
    assert np.array_equal(pts, aemu.points_scalar(qual, rot, move_center=move_center))
    c = aemu.centres(v, f)
    d = aemu.distances(c, pts)
    assert np.array_equal(d, aemu.distances_scalar(c, pts))
    for rad in (0.02, 0.05):
        assert not (np.abs(d - rad) < 1e-9).any()
        a = aemu.aggregate(d, pts[:, 3], "max", rad=rad)
        assert np.array_equal(a, aemu.max_scalar(d, pts[:, 3], rad))
        assert (a > 0).any() and (a == 0).any()


def test_points_follow_linspace_and_the_float32_threshold():
    R, size = 8, 0.3
    assert np.array_equal(aemu.lin(size, R), np.linspace(0, size, R))
    qual = np.zeros((R, R, R), F32)
    qual[1, 2, 3], qual[7, 7, 7], qual[0, 0, 1] = 0.75, 1.0, F32(0.5)       # 0.5 itself is not above th
    rot = np.zeros((R, R, R, 4), F32)
    rot[..., 3] = 1                                                          # identity: z axis (0, 0, 1)
    pts = aemu.points(qual, rot, size)
    t = np.linspace(0, size, R)
    off = float(F32(F32(1) * F32(0.05)) * F32(0.5))
    assert np.array_equal(pts, [[t[1], t[2], t[3] + off, 0.75], [size, size, size + off, 1.0]])
    assert np.array_equal(aemu.points(qual, rot, size, move_center=False)[:, :3], [[t[1], t[2], t[3]], [size, size, size]])


def test_normalise_and_the_aggregations_on_hand_values():
    q = np.array([0.6, 0.9])
    d = np.array([[0.01, 0.03], [0.03, 0.03], [0.01, 0.02]])
    assert np.array_equal(aemu.aggregate(d, q, "max"), [0.6, 0.0, 0.9])
    s = aemu.aggregate(d, q, "softmax")
    assert s[1] == 0.0 and abs(s[0] - 0.6) < 1e-12 and abs(s[2] - (0.6 * np.exp(90) + 0.9 * np.exp(135)) / (np.exp(90) + np.exp(135))) < 1e-12
    m = aemu.aggregate(d, q, "mean")
    assert abs(m[1] - 0.75) < 1e-15 and 0.6 < m[0] < 0.75
    with np.errstate(all="ignore"):
        assert np.isnan(aemu.aggregate(np.full((1, 2), 0.2), q, "mean", temp=1e4)).all()
    a = aemu.normalise(np.array([0.0, 0.5, 0.75, 1.0, 2.0, np.nan]))
    assert np.array_equal(a[:5], [0.0, 0.0, 0.5, 1.0, 1.0]) and np.isnan(a[5])
    assert np.array_equal(aemu.colours(a)[5], [0, 0, 0, 0]) and np.array_equal(aemu.colours(a)[0], [255, 245, 240, 255])
    assert np.array_equal(aemu.colours(a)[4], [103, 0, 13, 255])
    assert aemu.colour_index(np.array([0.5]))[0] == 16                       # 256 / 16, exactly


# ----------------------------------------------------------------------------------------------------------- colour table
def test_reds_table_is_the_same_in_the_package_the_library_and_the_restatement():
    t = visual.reds_table()
    assert t.shape == (256, 4) and np.array_equal(t, aemu.reds_table())
    lib_table = np.zeros((256, 4), np.uint8)
    _capi.lib().giga_affordance_colormap(lib_table.ctypes.data_as(ctypes.c_void_p))
    assert np.array_equal(lib_table, visual.to_uint8(t))
    assert np.abs(np.abs(255 * t - np.floor(255 * t)) - 0.5).min() > 1e-3    # no entry near a rounding tie of rint(255 c)
    _capi.lib().giga_affordance_colormap(None)                               # a null pointer is ignored


def test_reds_matches_matplotlib():
    mpl = pytest.importorskip("matplotlib")
    cmap = mpl.colormaps["Reds"]
    x = np.concatenate((np.linspace(0, 1, 4097), [1.0, -0.25, -1e-9, 1.5, 255 / 256, np.nextafter(1.0, 0), np.nan]))
    want = cmap(x)
    got = visual.reds(x)
    assert got.shape == want.shape == (len(x), 4)
    assert np.abs(got - want).max() < 1e-15
    assert np.array_equal(got[-1], [0, 0, 0, 0]) and np.array_equal(want[-1], [0, 0, 0, 0])
    assert np.array_equal(visual.to_uint8(got), np.rint(255 * want).astype(np.uint8))
    assert np.array_equal(got[4097], got[4096]) and np.array_equal(got[4098], got[0]) and np.array_equal(got[4100], got[4096])
    assert np.abs(visual.reds_table() - cmap(np.arange(256))).max() < 1e-15  # integer input indexes the table itself


# ---------------------------------------------------------------------------------------------------------------- gripper
GRASP = {"rotation": np.array([0.18257419, 0.36514837, 0.54772256, 0.73029674]), "translation": np.array([0.11, 0.17, 0.08]),
         "width": 0.06}


def signed_volume(v, f):
    a, b, c = (v[f[:, i]] for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def test_grasp2mesh_is_four_closed_outward_cylinders():
    m = visual.grasp2mesh(GRASP, 0.9)
    assert m.vertices.shape == (264, 3) and m.vertices.dtype == F32 and m.faces.shape == (512, 3) and m.faces.dtype == np.int64
    assert m.face_colors.shape == (512, 4) and (m.face_colors == np.array([0, 250, 0, 180], np.uint8)).all()
    v, f = visual.gripper_geometry(GRASP)
    assert v.dtype == np.float64 and np.array_equal(v.astype(F32), m.vertices) and np.array_equal(f, m.faces)
    # every edge is shared by exactly two faces, which run through it in opposite directions
    edges = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    directed = {}
    for a, b in edges:
        directed[(a, b)] = directed.get((a, b), 0) + 1
    assert all(n == 1 for n in directed.values()) and all((b, a) in directed for a, b in directed) and len(directed) == 3 * 512
    w, d = GRASP["width"], 0.05
    r = 0.1 * d
    want = 16 * np.sin(2 * np.pi / 32) * r * r * (d + d + d / 2 + w)
    assert abs(signed_volume(v, f) - want) <= 1e-12 * want
    for k in range(4):                                                       # each part alone is closed and outward too
        vk, fk = v[66 * k:66 * (k + 1)], f[128 * k:128 * (k + 1)] - 66 * k
        h = (d, d, d / 2, w)[k]
        assert fk.min() == 0 and fk.max() == 65
        part = 16 * np.sin(2 * np.pi / 32) * r * r * h
        assert abs(signed_volume(vk, fk) - part) <= 1e-12 * part


def test_grasp2mesh_parts_sit_where_the_pose_composition_puts_them():
    from scipy.spatial.transform import Rotation
    v, _ = visual.gripper_geometry(GRASP)
    Rm = Rotation.from_quat(GRASP["rotation"]).as_matrix()
    t, w, d = GRASP["translation"], GRASP["width"], 0.05
    quarter = Rotation.from_rotvec(np.pi / 2 * np.r_[1.0, 0.0, 0.0]).as_matrix()     # the palm's turn: z goes to -y
    local = [([0, -w / 2, d / 2], [0, 0, 1.0], d), ([0, w / 2, d / 2], [0, 0, 1.0], d), ([0, 0, -d / 4], [0, 0, 1.0], d / 2),
             ([0, 0, 0], quarter @ [0, 0, 1.0], w)]
    tol = 1e-13                                          # float64 throughout: a few ulps of 0.2, divided by a height of 0.025
    for k, (c, axis, h) in enumerate(local):
        part = v[66 * k:66 * (k + 1)]
        centre = Rm @ np.asarray(c, float) + t
        assert np.allclose(part[:2].mean(0), centre, atol=tol)               # the two cap centres straddle the part's centre
        got_axis = (part[1] - part[0]) / h
        want_axis = Rm @ np.asarray(axis, float)
        assert np.allclose(got_axis, want_axis, atol=tol)
        rim = part[2:] - centre                                              # rim vertices: 0.1 d from the axis, h / 2 along it
        assert np.allclose(np.abs(rim @ want_axis), h / 2, atol=tol)
        assert np.allclose(np.linalg.norm(rim - np.outer(rim @ want_axis, want_axis), axis=1), 0.1 * d, atol=tol)


# ------------------------------------------------------------------------------------------------------------ .ply and .obj
def read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = int([l for l in lines if l.startswith("element vertex")][0].split()[2])
    nf = int([l for l in lines if l.startswith("element face")][0].split()[2])
    props = [l for l in lines if l.startswith("property")]
    assert props == ["property float x", "property float y", "property float z", "property list uchar int vertex_indices",
                     "property uchar red", "property uchar green", "property uchar blue", "property uchar alpha"]
    v = np.frombuffer(body, "<f4", 3 * nv).reshape(nv, 3)
    rec = np.frombuffer(body, np.dtype([("n", "u1"), ("v", "<i4", (3,)), ("c", "u1", (4,))]), nf, 12 * nv)
    assert len(body) == 12 * nv + 17 * nf and (rec["n"] == 3).all()
    return v, rec["v"], rec["c"]


def read_obj(path):
    v, f = [], []
    for line in open(path):
        kind, *rest = line.split()
        (v if kind == "v" else f).append(rest)
        assert kind in ("v", "f")
    return np.asarray(v, np.float64).astype(F32), np.asarray(f, np.int64) - 1


def test_scene_composes_and_round_trips_through_ply_and_obj(tmp_path):
    v, f = remu.icosphere((0.15, 0.15, 0.1), 1 / 3.0, 1)
    rng = np.random.default_rng(0)
    base = visual.ColoredMesh(v, f, rng.integers(0, 256, (len(f), 4), dtype=np.uint8))
    scene = visual.Scene(base)
    scene.add_geometry(visual.grasp2mesh(GRASP), node_name="grasp_0")
    scene.add_geometry(visual.grasp2mesh(dict(GRASP, width=0.03)), node_name="grasp_1")
    assert scene.ranges == {"scene": (0, 80), "grasp_0": (80, 592), "grasp_1": (592, 1104)}
    assert scene.vertices.dtype == F32 and scene.faces.dtype == np.int64 and scene.face_colors.dtype == np.uint8
    assert len(scene.vertices) == len(v) + 2 * 264 and scene.faces[80:].min() == len(v) and scene.faces.max() == len(scene.vertices) - 1
    faces, colours = scene.geometry("grasp_1")
    assert (colours == np.array([0, 250, 0, 180], np.uint8)).all() and faces.min() == len(v) + 264
    with pytest.raises(ValueError):
        scene.add_geometry(base, node_name="scene")
    pv, pf, pc = read_ply(scene.export(tmp_path / "scene.ply"))
    assert np.array_equal(pv, scene.vertices) and np.array_equal(pf, scene.faces) and np.array_equal(pc, scene.face_colors)
    ov, of = read_obj(scene.export(str(tmp_path / "scene.obj")))
    assert np.array_equal(ov, scene.vertices) and np.array_equal(of, scene.faces)
    with pytest.raises(ValueError):
        scene.export(tmp_path / "scene.stl")
    with pytest.raises(ValueError):
        visual.ColoredMesh(v, f, np.zeros((3, 4), np.uint8))


# --------------------------------------------------------------------------------------------- ABI validation without a device
_BUF = (ctypes.c_double * 256)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 40


def _params(**kw):
    p = dict(size=0.3, th=0.5, temp=150.0, rad=0.02, finger_depth=0.05, finger_offset=0.5, move_center=1, aggregation=0)
    p.update(kw)
    return _capi.AffordanceParams(*[p[k] for k in ("size", "th", "temp", "rad", "finger_depth", "finger_offset", "move_center", "aggregation")])


def _arr(values):
    return NUL if values is None else (ctypes.c_int32 * len(values))(*values)


def _points(qual=A, rot=A, B=1, R=8, prm=None, null_prm=False, points=A, counts=A, ws=A, ws_bytes=BIG):
    prm = _params(**(prm or {}))
    return _capi.lib().giga_affordance_points(qual, rot, B, R, NUL if null_prm else ctypes.byref(prm), points, counts, ws, ws_bytes, NUL)


def _faces(vertices=A, voffs=(0, 8), triangles=A, toffs=(0, 12), points=A, counts=A, B=1, R=8, prm=None, null_prm=False, aff=A, rgba=A,
           ws=A, ws_bytes=BIG):
    prm = _params(**(prm or {}))
    return _capi.lib().giga_affordance_faces(vertices, _arr(voffs), triangles, _arr(toffs), points, counts, B, R,
                                             NUL if null_prm else ctypes.byref(prm), aff, rgba, ws, ws_bytes, NUL)


BAD_PARAMS = [dict(aggregation=3), dict(aggregation=-1), dict(aggregation=256 + 3), dict(aggregation=512)] + \
             [{k: x} for k in ("size", "th", "temp", "rad", "finger_depth", "finger_offset") for x in (float("nan"), float("inf"))]


@pytest.mark.parametrize("kwargs, code", [
    (dict(B=-1), -1), (dict(B=_capi.MAX_SCENES + 1), -7), (dict(R=1), -1), (dict(R=0), -1), (dict(R=_capi.TSDF_MAX_R + 1), -1),
    (dict(null_prm=True), -1), (dict(qual=NUL), -1), (dict(rot=NUL), -1), (dict(points=NUL), -1), (dict(counts=NUL), -1),
    (dict(ws=NUL), -1), (dict(ws_bytes=100), -4), (dict(ws_bytes=0), -4),
    (dict(B=0), 0), (dict(B=0, qual=NUL, rot=NUL, points=NUL, counts=NUL, ws=NUL), 0),
] + [(dict(prm=p), -1) for p in BAD_PARAMS])
def test_affordance_points_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _points(**kwargs) == code


@pytest.mark.parametrize("kwargs, code", [
    (dict(B=-1), -1), (dict(B=_capi.MAX_SCENES + 1), -7), (dict(R=1), -1), (dict(R=_capi.TSDF_MAX_R + 1), -1), (dict(null_prm=True), -1),
    (dict(voffs=None), -1), (dict(toffs=None), -1), (dict(voffs=(1, 8)), -1), (dict(toffs=(2, 12)), -1), (dict(voffs=(0, -8)), -1),
    (dict(toffs=(0, -1)), -1), (dict(B=2, voffs=(0, 8, 4), toffs=(0, 12, 12)), -1), (dict(B=2, voffs=(0, 8, 8), toffs=(0, 12, 6)), -1),
    (dict(vertices=NUL), -1), (dict(triangles=NUL), -1), (dict(points=NUL), -1), (dict(counts=NUL), -1), (dict(aff=NUL), -1),
    (dict(rgba=NUL), -1), (dict(ws=NUL), -1), (dict(ws_bytes=100), -4),
    (dict(B=0), 0), (dict(toffs=(0, 0), triangles=NUL, points=NUL, counts=NUL, aff=NUL, rgba=NUL, ws=NUL), 0),   # no faces: nothing to do
] + [(dict(prm=p), -1) for p in BAD_PARAMS])
def test_affordance_faces_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _faces(**kwargs) == code


def test_affordance_is_exported_and_declared():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_affordance_points", "giga_affordance_faces", "giga_affordance_workspace_bytes", "giga_affordance_colormap"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    for name, value in _capi.AFFORDANCE.items():
        assert value == int(hdr.split("#define GIGA_AFFORDANCE_" + name.upper())[1].split()[0])
    assert _capi.AFFORDANCE_DENSE == int(hdr.split("#define GIGA_AFFORDANCE_DENSE")[1].split()[0])
    assert ctypes.sizeof(_capi.AffordanceParams) == 56
    assert L.giga_affordance_workspace_bytes(0, 8, 10) == 0 and L.giga_affordance_workspace_bytes(1, 1, 10) == 0
    assert L.giga_affordance_workspace_bytes(1, 8, -1) == 0 and L.giga_affordance_workspace_bytes(_capi.MAX_SCENES + 1, 8, 10) == 0
    small, large = L.giga_affordance_workspace_bytes(1, 8, 10), L.giga_affordance_workspace_bytes(3, 40, 10)
    assert small >= 1024 + 3 * 8 + 4 * 2 + 4 * 4 * 512 and large >= 3 * 4 * 4 * 64000
    assert L.giga_affordance_workspace_bytes(1, 128, 10) < 4 * 128 ** 3        # beyond 2^20 voxels: no sort buffers


# ------------------------------------------------------------------------------------------------------------- host logic
def test_planner_with_visualize_needs_the_scene_mesh():
    planner = VGNImplicit.__new__(VGNImplicit)          # the host logic alone: no device, no network
    planner.visualize = True
    with pytest.raises(ValueError):
        planner(object())
    with pytest.raises(ValueError):
        planner(object(), None, {"rad": 0.05})


def test_affordance_needs_a_device_and_known_arguments():
    import torch
    import giga_amd
    v, f = remu.plane_mesh(0.05, 0.3)
    q, r = torch.zeros((8, 8, 8)), torch.zeros((8, 8, 8, 4))
    with pytest.raises(_capi.GigaHipError):
        visual.affordance_faces(q, r, (v, f))
    with pytest.raises(_capi.GigaHipError):
        visual.affordance_faces(q.numpy(), r.numpy(), (v, f))
    with pytest.raises(ValueError):
        visual.affordance_faces(q, r, (v, f), aggregation="median")
    assert giga_amd.affordance_visual is visual.affordance_visual and giga_amd.grasp2mesh is visual.grasp2mesh
    assert giga_amd.Scene is visual.Scene and giga_amd.affordance_faces is visual.affordance_faces
