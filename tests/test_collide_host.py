"""giga_mesh_collide on the host: the numpy restatement against exact rational arithmetic, hand cases of the header's rule, and the
C entry's argument checks, which answer before the first HIP call (null device pointers)."""
import ctypes
import os

import numpy as np
import pytest

import collide_emu as cemu
from giga_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ------------------------------------------------------------------------------------------- restatement against exact signs
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_restatement_equals_the_exact_decision_on_every_triangle_pair(seed):
    """The GPU test's random inputs hold no knife-edge configuration: float64 decides every triangle pair as exact arithmetic
    does, so the device is held to a decision that does not hang on a rounding."""
    bodies = cemu.random_bodies(seed)
    tris = [cemu.usable_triangles(v, f)[0] for v, f in bodies]
    assert [len(t) for t in tris] == [12] * 8 + [80] * 4
    disagreements = pairs = hits = 0
    for a in range(len(bodies)):
        for b in range(a + 1, len(bodies)):
            got = cemu.tri_tri(tris[a][:, None], tris[b][None])
            want = cemu.tri_tri_exact(tris[a], tris[b])
            disagreements += int((got != want).sum())
            pairs += got.size
            hits += int(want.sum())
    assert pairs == 28 * 144 + 32 * 960 + 6 * 6400 and hits > 100           # the bodies do overlap
    assert disagreements == 0


# ------------------------------------------------------------------------------------------------------------------ hand cases
def _tri(*corners):
    return np.asarray(corners, F32)


def _bodies_hit(A, B):
    f = np.array([[0, 1, 2]], np.int32)
    return bool(cemu.mesh_collide([(A, f), (B, f)], [(0, 1)])[0]), bool(cemu.mesh_collide([(A, f), (B, f)], [(1, 0)])[0])


def test_two_triangles_crossing_and_two_disjoint():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    B = _tri((0.2, 0.2, -0.5), (0.2, 0.2, 0.5), (0.9, 0.9, 0.5))
    assert cemu.tri_tri(A, B) and cemu.tri_tri(B, A) and _bodies_hit(A, B) == (True, True)
    assert bool(cemu.tri_tri_exact(A[None], B[None])[0, 0])
    C = B + F32(2.0)
    assert not cemu.tri_tri(A, C) and _bodies_hit(A, C) == (False, False)
    D = _tri((0.2, 0.2, 0.1), (0.3, 0.2, 0.6), (0.2, 0.3, 0.5))             # boxes overlap, all of D above A's plane
    assert not cemu.tri_tri(A, D) and _bodies_hit(A, D) == (False, False)


def test_sharing_only_a_vertex_is_a_hit_because_zero_counts():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    B = _tri((0, 0, 0), (-1, 0, 1), (0, -1, 1))
    assert cemu.tri_tri(A, B) and _bodies_hit(A, B) == (True, True)
    assert bool(cemu.tri_tri_exact(A[None], B[None])[0, 0])


def test_coplanar_overlap_is_not_detected_by_definition():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    B = _tri((0.1, 0.1, 0), (0.9, 0.2, 0), (0.2, 0.9, 0))
    assert not cemu.tri_tri(A, B) and _bodies_hit(A, B) == (False, False)
    assert not cemu.tri_tri_exact(A[None], B[None])[0, 0]


def test_nan_vertex_and_index_outside_the_body_intersect_nothing():
    A = _tri((0, 0, 0), (1, 0, 0), (0, 1, 0))
    B = _tri((0.2, 0.2, -0.5), (0.2, 0.2, 0.5), (0.9, 0.9, 0.5))
    bad = B.copy()
    bad[1, 2] = np.nan
    assert not cemu.tri_tri(A, bad) and not cemu.tri_tri(bad, A)          # the rule itself: a NaN determinant misses
    assert _bodies_hit(A, bad) == (False, False)
    f_ok, f_out = np.array([[0, 1, 2]], np.int32), np.array([[0, 1, 3]], np.int32)
    assert not cemu.mesh_collide([(A, f_ok), (B, f_out)], [(0, 1)])[0]
    assert not cemu.mesh_collide([(A, f_ok), (B, np.array([[0, -1, 2]], np.int32))], [(0, 1)])[0]
    # a body keeps its usable triangles
    both = np.concatenate((bad, B)), np.array([[0, 1, 2], [3, 4, 5]], np.int32)
    assert cemu.mesh_collide([(A, f_ok), both], [(0, 1)])[0]


def test_l_prism_is_closed_and_its_notch_is_empty():
    v, f = cemu.l_prism()
    assert v.shape == (12, 3) and f.shape == (20, 3)
    edges = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
    assert (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()
    vol = (cemu.orient(np.zeros((len(f), 3)), v[f[:, 0]].astype(np.float64), v[f[:, 1]].astype(np.float64), v[f[:, 2]].astype(np.float64)) / 6).sum()
    assert abs(vol - (0.1 * 0.1 - 0.06 * 0.06) * 0.05) < 1e-9               # outward winding, the L's area times the height
    inside_notch = cemu.box_mesh((0.05, 0.05, 0.01), (0.09, 0.09, 0.04))
    assert not cemu.pair_hit((v, f), inside_notch)
    assert cemu.pair_hit((v, f), cemu.box_mesh((0.03, 0.05, 0.01), (0.09, 0.09, 0.04)))


# -------------------------------------------------------------------------------------------------------------- the C entry
def test_symbols_are_declared_exported_and_built():
    L = _capi.lib()
    header = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    for name in ("giga_mesh_collide", "giga_mesh_collide_workspace_bytes"):
        assert hasattr(L, name) and name in _capi.EXPORTS and name + "(" in header
    assert "giga_collide.o" in open(os.path.join(ROOT, "giga_amd", "csrc", "Makefile")).read()
    raw = ctypes.CDLL(_capi.LIB_PATH)                                      # the dynamic symbol table itself, no argtypes
    assert raw.giga_mesh_collide and raw.giga_mesh_collide_workspace_bytes
    assert L.giga_abi_version() == 3


_BUF = (ctypes.c_double * 64)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 30


def _ints(*xs):
    return np.ascontiguousarray(xs, np.int32)


def _collide(v=A, vo=(0, 3, 6), t=A, fo=(0, 1, 2), M=2, pairs=(0, 1), P=1, hit=A, ws=A, ws_bytes=BIG):
    keep = [_ints(*x) if x is not None else None for x in (vo, fo, pairs)]
    args = [k.ctypes.data_as(ctypes.c_void_p) if k is not None else NUL for k in keep]
    return _capi.lib().giga_mesh_collide(v, args[0], t, args[1], M, args[2], P, hit, ws, ws_bytes, NUL)


@pytest.mark.parametrize("kwargs, code", [
    (dict(M=-1), -1), (dict(P=-1), -1),                                     # negative count
    (dict(v=NUL), -1), (dict(t=NUL), -1), (dict(vo=None), -1), (dict(fo=None), -1), (dict(pairs=None), -1), (dict(ws=NUL), -1),
    (dict(vo=(1, 3, 6)), -1), (dict(fo=(0, 2, 1)), -1), (dict(vo=(0, 6, 3)), -1),
    (dict(pairs=(0, 2)), -1), (dict(pairs=(-1, 1)), -1), (dict(pairs=(2, 0)), -1), (dict(pairs=(1, 1)), -1),
    (dict(P=2, pairs=(0, 1, 1, 1)), -1),
    (dict(ws_bytes=255), -4),
    (dict(hit=NUL), -6),
    (dict(M=_capi.MAX_SCENES + 1), -7),
    (dict(M=0), 0), (dict(P=0), 0), (dict(P=0, hit=NUL), 0), (dict(M=0, pairs=(5, 5)), 0),
])
def test_collide_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _collide(**kwargs) == code


def test_workspace_sizes():
    L = _capi.lib()
    assert L.giga_mesh_collide_workspace_bytes(0, 10) == 0
    assert L.giga_mesh_collide_workspace_bytes(_capi.MAX_SCENES + 1, 10) == 0
    assert L.giga_mesh_collide_workspace_bytes(4, -1) == 0
    # two offset arrays, the pairs and six floats per body, each on a 256-byte boundary
    assert L.giga_mesh_collide_workspace_bytes(384, 2112) >= 2 * 385 * 4 + 2112 * 8 + 384 * 24
    assert L.giga_mesh_collide_workspace_bytes(1, 0) % 256 == 0 and L.giga_mesh_collide_workspace_bytes(1, 0) > 0


def test_mesh_bounds_batch_and_cpu_tensors():
    import torch

    from giga_amd import collision
    v, f = cemu.box_mesh((0, 1, 2), (3, 5, 7))
    bounds = collision.mesh_bounds_batch([(v, f), (torch.from_numpy(v) + 1, torch.from_numpy(f)), (np.zeros((0, 3), F32), f[:0])])
    assert bounds.shape == (3, 2, 3) and bounds.dtype == F32
    assert bounds[0].tolist() == [[0, 1, 2], [3, 5, 7]] and bounds[1].tolist() == [[1, 2, 3], [4, 6, 8]]
    assert np.isposinf(bounds[2, 0]).all() and np.isneginf(bounds[2, 1]).all()
    with pytest.raises(_capi.GigaHipError):
        collision.mesh_collide([(torch.from_numpy(v), torch.from_numpy(f))] * 2, [(0, 1)])
    import giga_amd
    assert giga_amd.mesh_collide is collision.mesh_collide and giga_amd.mesh_bounds_batch is collision.mesh_bounds_batch
