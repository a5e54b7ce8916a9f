"""CPU tests of the grasp candidates: the new symbols and their argument checks, `reduce_outcomes` and the frame against scipy
itself, closed forms of the normal restatement, the sampler of the emulation, and the file-writing half of `write_geo_dataset`."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import candidates_emu as cand
from candidates_emu import LOWER, UPPER, fake_execute, frame_normals, sampler_cloud
from giga_amd import _capi, candidates, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000                                # a device address that no check dereferences
SYMBOLS = ("giga_tsdf_cloud_emit_oriented", "giga_grasp_candidates_workspace_bytes", "giga_grasp_candidates")


# ------------------------------------------------------------------------------------------------ symbols and argument checks
def test_symbols_are_declared_exported_and_in_the_signature_table():
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    lib = _capi.lib()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _capi._SIGNATURES and name in _capi.EXPORTS and hasattr(lib, name)
    assert "giga_candidates.o" in open(os.path.join(ROOT, "giga_amd", "csrc", "Makefile")).read()
    assert lib.giga_abi_version() == 3
    assert _capi.CANDIDATES_MAX_ROTATIONS == int(re.search(r"#define GIGA_CANDIDATES_MAX_ROTATIONS (\d+)", hdr).group(1)) == 32


def test_emit_oriented_refuses_bad_arguments_before_any_device_call():
    lib = _capi.lib()
    ws = lib.giga_tsdf_cloud_workspace_bytes(2, 8)
    assert ws > 0

    def call(tsdf=FAKE, weight=FAKE, B=2, R=8, length=0.3, workspace=FAKE, nbytes=ws, points=FAKE, normals=FAKE, cap=10):
        return lib.giga_tsdf_cloud_emit_oriented(tsdf, weight, B, R, length, workspace, nbytes, points, normals, cap, None, None)
    assert call(B=0) == 0
    assert call(B=-1) == -1 and call(R=1) == -1 and call(R=_capi.TSDF_MAX_R + 1) == -1
    assert call(length=0.0) == -1 and call(length=float("nan")) == -1 and call(length=float("inf")) == -1
    assert call(tsdf=None) == -1 and call(weight=None) == -1 and call(workspace=None) == -1
    assert call(points=None) == -6 and call(normals=None) == -6
    assert call(nbytes=ws - 1) == -4
    assert call(B=_capi.MAX_SCENES + 1) == -7


def test_grasp_candidates_refuses_bad_arguments_before_any_device_call():
    lib = _capi.lib()
    offsets = np.array([0, 5, 5, 9], np.int32)
    ids = np.arange(3, dtype=np.uint32)
    lower, upper = np.zeros(3), np.ones(3)
    table = candidates.yaw_table(6)
    ws = lib.giga_grasp_candidates_workspace_bytes(3, 9, 6)
    assert ws > 0 and lib.giga_grasp_candidates_workspace_bytes(3, 9, 0) == 0 and lib.giga_grasp_candidates_workspace_bytes(3, 9, 33) == 0

    def call(points=FAKE, normals=FAKE, offsets=offsets, ids=ids, B=3, K=4, lower=lower, upper=upper, finger_depth=0.05, eps=0.1,
             table=table, Y=6, pos=FAKE, quat=FAKE, index=FAKE, counts=FAKE, workspace=FAKE, nbytes=ws):
        host = [None if a is None else _capi.host_ptr(a) for a in (offsets, ids, lower, upper, table)]
        return lib.giga_grasp_candidates(points, normals, host[0], host[1], B, K, host[2], host[3], finger_depth, eps, host[4], Y, 7,
                                         pos, quat, index, counts, workspace, nbytes, None)
    assert call(B=0) == 0 and call(K=0) == 0
    assert call(B=-1) == -1 and call(K=-1) == -1 and call(Y=0) == -1 and call(Y=33) == -1
    assert call(B=_capi.MAX_SCENES + 1) == -7
    assert call(finger_depth=float("nan")) == -1 and call(eps=float("inf")) == -1
    assert call(offsets=np.array([1, 5, 5, 9], np.int32)) == -1 and call(offsets=np.array([0, 5, 4, 9], np.int32)) == -1
    assert call(offsets=None) == -1 and call(ids=None) == -1 and call(lower=None) == -1 and call(upper=None) == -1 and call(table=None) == -1
    assert call(lower=np.array([0.0, np.nan, 0.0])) == -1 and call(upper=np.array([np.inf, 1.0, 1.0])) == -1
    bad = table.copy()
    bad[5, 1] = np.nan
    assert call(table=bad) == -1
    assert call(points=None) == -1 and call(normals=None) == -1 and call(workspace=None) == -1
    for name in ("pos", "quat", "index", "counts"):
        assert call(**{name: None}) == -6
    assert call(nbytes=ws - 1) == -4


def test_python_wrapper_refuses_cpu_tensors_and_bad_shapes():
    import torch
    p = torch.zeros((4, 3))
    with pytest.raises(_capi.GigaHipError):
        candidates.grasp_candidates(p, p, [0, 4], 3, lower=np.zeros(3), upper=np.ones(3))
    with pytest.raises(ValueError):
        candidates.yaw_table(0)
    with pytest.raises(ValueError):
        candidates.yaw_table(33)
    lower, upper = candidates.workspace_bounds(0.3, 0.05)
    assert np.array_equal(lower, np.r_[0.02, 0.02, 0.05 + 0.005]) and np.array_equal(upper, np.r_[0.3 - 0.02, 0.3 - 0.02, 0.3])
    import giga_amd
    for name in ("workspace_bounds", "grasp_candidates", "reduce_outcomes", "label_scenes"):
        assert getattr(giga_amd, name) is getattr(candidates, name)


# ------------------------------------------------------------------------------------------------ reduce_outcomes against scipy
def test_reduce_outcomes_equals_find_peaks_for_every_pattern():
    """generate_data_parallel.py:168-179 with scipy's own find_peaks, for all outcome patterns of 1 .. 8 yaws."""
    from scipy import signal
    for Y in range(1, 9):
        patterns = np.array(list(itertools.product((0, 1), repeat=Y)), np.int64)
        K = len(patterns)
        rng = np.random.default_rng(Y)
        widths, quat = rng.uniform(0.0, 0.08, (K, Y)), rng.normal(size=(K, Y, 4))
        q, w, label = candidates.reduce_outcomes(patterns, widths, quat)
        for k, s in enumerate(patterns):
            if s.sum():
                peaks, properties = signal.find_peaks(x=np.r_[0, s.astype(float), 0], height=1, width=1)
                want = peaks[np.argmax(properties["widths"])] - 1
            else:
                want = Y - 1                                                # the loop variables' last values
            assert np.array_equal(q[k], quat[k, want]) and w[k] == widths[k, want] and label[k] == s.max(), (Y, s, want)


def test_reduce_outcomes_refuses_mismatched_shapes():
    with pytest.raises(ValueError):
        candidates.reduce_outcomes(np.zeros((2, 3)), np.zeros((2, 4)), np.zeros((2, 3, 4)))


# ------------------------------------------------------------------------------------------------ frame and yaw against scipy
def test_frame_and_yaw_quaternions_equal_scipy():
    """The emulation against Rotation.from_matrix(M) * Rotation.from_euler("z", yaw) of the installed scipy, M built the way
    generate_data_parallel.py:149-155 builds it (columns not normalised), up to the quaternion's sign, to 1e-12 per component.
    Written against scipy 1.15.3, which returns the rotation of M with every column normalised; a scipy that orthogonalises M
    differently would fail here."""
    import scipy
    from scipy.spatial.transform import Rotation
    N = frame_normals()
    Y = 6
    got = cand.yaw_quats(cand.frame_quat(N), cand.yaw_table(Y))
    yaws = np.linspace(0.0, np.pi, Y)
    worst, switched = 0.0, 0
    for k, normal in enumerate(N):
        z_axis = -normal / np.linalg.norm(normal)
        x_axis = np.r_[1.0, 0.0, 0.0]
        if np.isclose(np.abs(np.dot(x_axis, z_axis)), 1.0, 1e-4):
            x_axis = np.r_[0.0, 1.0, 0.0]
            switched += 1
        y_axis = np.cross(z_axis, x_axis)
        x_axis = np.cross(y_axis, z_axis)
        R = Rotation.from_matrix(np.vstack((x_axis, y_axis, z_axis)).T)
        for j, yaw in enumerate(yaws):
            want = (R * Rotation.from_euler("z", yaw)).as_quat()
            worst = max(worst, min(np.abs(got[k, j] - want).max(), np.abs(got[k, j] + want).max()))
    print("scipy", scipy.__version__, "largest quaternion component difference", worst, "frames on the y axis", switched)
    assert worst <= 1e-12, f"scipy {scipy.__version__} (written against 1.15.3): {worst}"
    assert switched == 2 + 4 * 3                   # +-x, and the 0.9999 and 0.99991 normals; 0.99989 stays on x


def test_frame_z_axis_is_minus_the_normal():
    N = frame_normals()
    x, y, z = cand.frame_axes(N)
    assert np.abs(z + N / np.linalg.norm(N, axis=1)[:, None]).max() < 1e-15
    for a, b in ((x, y), (y, z), (x, z)):
        assert np.abs((a * b).sum(1)).max() < 1e-12
    assert np.abs(np.linalg.norm(x, axis=1) - 1).max() < 1e-15 and np.abs(np.linalg.norm(y, axis=1) - 1).max() < 1e-15


# ------------------------------------------------------------------------------------------------ closed forms of the normal
def test_affine_volume_has_the_unit_gradient_at_every_crossing():
    """tsdf = (3 x + 2 y - 6 z + 0.5) / 128 in cell indices is exact in float32 and stays inside +-0.98; the weights keep the
    crossings two cells away from the boundary, where every voxel a normal reads lies inside the volume.  The trilinear
    interpolation of an affine function is the function, so the float64 normal is (3, 2, -6) / 7 up to rounding."""
    R, length = 12, 0.3
    x, y, z = np.meshgrid(np.arange(R), np.arange(R), np.arange(R), indexing="ij")
    tsdf = ((3 * x + 2 * y - 6 * z + 0.5) / 128).astype(np.float32)
    assert np.array_equal(tsdf.astype(np.float64) * 128, 3 * x + 2 * y - 6 * z + 0.5) and np.abs(tsdf).max() < 0.98
    weight = np.zeros((R, R, R), np.float32)
    weight[2:R - 2, 2:R - 2, 2:R - 2] = 1
    p = cand.cloud_points64(tsdf, weight, length)
    assert len(p) > 100
    n = cand.normals64_at(tsdf, p, length)
    assert np.abs(n - np.array([3.0, 2.0, -6.0]) / 7.0).max() <= 1e-12
    points, normals = cand.cloud_oriented(tsdf, weight, length)
    assert np.array_equal(normals, n.astype(np.float32)) and len(points) == len(p)


def test_constant_neighbourhood_has_the_zero_normal():
    R, length = 6, 0.3
    tsdf = np.full((R, R, R), 0.25, np.float32)
    p = np.array([[0.15, 0.15, 0.15], [0.13, 0.17, 0.12]])
    assert np.array_equal(cand.normals64_at(tsdf, p, length), np.zeros((2, 3)))
    assert np.array_equal(cand.normals_at(tsdf, p, length).view(np.uint32), np.zeros((2, 3), np.uint32))       # +0.0


def test_crossing_in_cell_zero_reads_zeros_outside_the_volume():
    """+0.5 in the first x layer, -0.5 behind it: the crossing of cell 0 lies at x = 1.0 voxel.  T(p - g) is taken at
    s = 0.01 - 0.5 = -0.49: 0.49 of the voxel -1, which counts 0.0, and 0.51 of +0.5.  Had the outside repeated the edge, the
    difference would be -1.0."""
    R, length = 4, 0.4
    v = length / R
    tsdf = np.full((R, R, R), -0.5, np.float32)
    tsdf[0] = 0.5
    weight = np.ones((R, R, R), np.float32)
    p = cand.cloud_points64(tsdf, weight, length)
    at = np.nonzero((np.abs(p[:, 0] - v) < 1e-12) & (np.abs(p[:, 1] - 1.5 * v) < 1e-12) & (np.abs(p[:, 2] - 1.5 * v) < 1e-12))[0]
    assert len(at) == 1
    n = cand.gradient_at(tsdf, p[at], length)[0]
    assert abs(n[0] - (-0.5 - 0.51 * 0.5)) < 1e-12 and abs(n[1]) < 1e-12 and abs(n[2]) < 1e-12
    assert np.abs(cand.normals64_at(tsdf, p[at], length)[0] - [-1.0, 0.0, 0.0]).max() < 1e-12


# ------------------------------------------------------------------------------------------------ sampler emulation
def test_sampler_draws_only_eligible_points_at_a_depth_inside_its_range():
    rng = np.random.default_rng(0)
    eligible_at = sorted(rng.choice(200, 37, replace=False).tolist())
    points, normals = sampler_cloud(rng, 200, eligible_at)
    assert np.nonzero(cand.eligible(points, normals, LOWER, UPPER))[0].tolist() == eligible_at
    pos, quat, index, E, depth = cand.candidates(points, normals, 500, LOWER, UPPER, scene_id=3, seed=11)
    assert E == 37 and set(index.tolist()) <= set(eligible_at) and len(set(index.tolist())) > 30
    lo, hi = -0.1 * 0.05, 1.1 * 0.05
    assert depth.min() >= lo and depth.max() <= hi and depth.min() < lo + 0.005 and depth.max() > hi - 0.005
    P, N = points[index].astype(np.float64), normals[index].astype(np.float64)
    assert np.abs((pos - P) - depth[:, None] * N).max() < 1e-16
    assert quat.shape == (500, 6, 4) and np.abs(np.linalg.norm(quat, axis=2) - 1).max() < 1e-15
    assert cand.candidates(points[:0], normals[:0], 5, LOWER, UPPER, 0, 0)[3] == 0


def test_sampler_is_uniform_over_the_eligible_points():
    """8 eligible points, 4096 candidates: every point is drawn 512 +- 6 standard deviations of the binomial (sd 21.2) times,
    386 .. 638.  The draws are a fixed function of (seed, scene id): seed 1, scene 0 is one for which this holds -- as it must
    for all but about 1.6e-8 of the seeds if the generator is uniform."""
    rng = np.random.default_rng(1)
    eligible_at = [3, 10, 11, 40, 41, 42, 77, 99]
    points, normals = sampler_cloud(rng, 100, eligible_at)
    index = cand.candidates(points, normals, 4096, LOWER, UPPER, scene_id=0, seed=1)[2]
    drawn = np.bincount(index, minlength=100)
    print("draws per eligible point", drawn[eligible_at].tolist())
    assert drawn.sum() == 4096 and drawn[eligible_at].sum() == 4096
    assert drawn[eligible_at].min() >= 386 and drawn[eligible_at].max() <= 638


# ------------------------------------------------------------------------------------------------ grasps.csv
def test_grasps_csv_rows_with_an_executor_and_the_placeholder_without(tmp_path):
    rng = np.random.default_rng(2)
    ids = [scenes.scene_id(4, s) for s in range(3)]
    labelled, K = [], 40
    for s in range(3):
        if s == 1:
            labelled.append(None)                                           # a scene without an eligible point
            continue
        points, normals = sampler_cloud(rng, 60, range(0, 60, 2))
        pos, quat = cand.candidates(points, normals, K, LOWER, UPPER, scene_id=s, seed=4)[:2]
        outcomes, widths = fake_execute(s, pos, quat, 0.08)
        q, w, label = candidates.reduce_outcomes(outcomes, widths, quat)
        labelled.append((pos, q, w, label))
    assert scenes.write_grasps_csv(tmp_path, ids, labelled) == [ids[1]]
    lines = open(tmp_path / "grasps.csv").read().splitlines()
    assert lines[0] == "scene_id,qx,qy,qz,qw,x,y,z,width,label" and len(lines) == 1 + 2 * K
    import pandas as pd
    df = pd.read_csv(tmp_path / "grasps.csv", float_precision="round_trip")      # (the rows hold repr(float): every bit)
    assert list(df.columns) == ["scene_id", "qx", "qy", "qz", "qw", "x", "y", "z", "width", "label"]
    assert df["scene_id"].tolist() == [ids[0]] * K + [ids[2]] * K
    for sid, entry in ((ids[0], labelled[0]), (ids[2], labelled[2])):
        rows = df[df["scene_id"] == sid]
        assert np.array_equal(rows[["x", "y", "z"]].to_numpy(), entry[0]) and np.array_equal(rows[["qx", "qy", "qz", "qw"]].to_numpy(), entry[1])
        assert np.array_equal(rows["width"].to_numpy(), entry[2]) and np.array_equal(rows["label"].to_numpy(), entry[3])
        assert 0 < rows["label"].sum() < K and set(rows["label"]) == {0, 1}
    # without an executor: the placeholder rows, as before
    assert scenes.write_grasps_csv(tmp_path, ids) == []
    assert open(tmp_path / "grasps.csv").read().splitlines()[1:] == [sid + ",0.0,0.0,0.0,1.0,0.15,0.15,0.15,0.0,0" for sid in ids]


def test_command_line_names_an_executor():
    from giga_amd import generate_scenes
    base = ["--object-set", "o", "--raw", "r", "--dataset", "d"]
    args = generate_scenes.build_parser().parse_args(base)
    assert (args.executor, args.grasps_per_scene, args.num_rotations) == (None, 120, 6)
    args = generate_scenes.build_parser().parse_args(base + ["--executor", "candidates_emu:fake_execute", "--grasps-per-scene", "7"])
    assert candidates.resolve_executor(args.executor) is fake_execute and args.grasps_per_scene == 7
    with pytest.raises(ValueError):
        candidates.resolve_executor("no_colon")


def test_scene_views_depend_on_seed_and_scene_alone():
    a, b = candidates.scene_views(3, 5), candidates.scene_views(3, 5)
    assert a.shape == (6, 4, 4) and np.array_equal(a, b) and not np.array_equal(a, candidates.scene_views(3, 6))
    eye = np.stack([-e[:3, :3].T @ e[:3, 3] for e in a]) - [0.15, 0.15, 0.0]       # camera centres about the origin of the views
    r = np.linalg.norm(eye, axis=1)
    assert (r >= 1.6 * 0.3 - 1e-12).all() and (r <= 2.4 * 0.3 + 1e-12).all()
    assert (np.arccos(eye[:, 2] / r) <= np.pi / 4 + 1e-12).all()
