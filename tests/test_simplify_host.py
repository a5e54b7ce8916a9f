"""CPU tests of the mesh simplification: the float64 restatements of the reference's quadric edge collapse (tests/simplify_emu.py:
the header's sequential loop, and the round schedule of csrc/giga_simplify.hip) against the reference's own Simplify.h driven
stand-alone (tests/golden/g20_simplify.npz, written by tools/make_simplify_goldens.py), the C ABI's argument checks and the
generator's argument behaviour."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import simplify_emu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tetra_2", "octa_4", "ico2_160", "ico2_32", "ico2_6", "torus_576", "torus_114", "torus_7", "cap_404", "cap_80", "cap_7",
         "mc17_f2", "mc17_f10", "mc33_f2", "mc33_f10", "unref_40", "ico2_keep", "unref_keep", "ico1_0"]


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_simplify.npz")


def _case(g20, name):
    return (g20[name + "_vertices_in"], g20[name + "_faces_in"], int(g20[name + "_target"]), float(g20[name + "_agressiveness"]),
            g20[name + "_vertices"], g20[name + "_faces"])


def test_the_fixture_holds_the_cases_it_must(g20):
    assert list(g20["names"]) == NAMES
    stats = {n: g20[n + "_stats"] for n in NAMES}                       # iterations, rounds, repeated passes, longest pass
    for n in NAMES:
        v, f, target, _, ov, of = _case(g20, n)
        assert v.dtype == np.float32 and f.dtype == np.int32 and ov.dtype == np.float64 and of.dtype == np.int32
        assert len(of) <= max(target, 0) or stats[n][0] == 100 or target >= len(f)     # above the target only after all 100 iterations
    assert any(s[2] > 0 for s in stats.values())                        # a budget met by a collapse that is not its pass's last
    assert stats["torus_7"][0] == 100 and len(g20["torus_7_faces"]) > 7     # cannot reach its target: ends above it
    assert stats["ico2_32"][0] > 10 and stats["cap_80"][0] > 10         # past the compactions of iterations 5 and 10
    v, f = g20["cap_404_vertices_in"], g20["cap_404_faces_in"]          # an open mesh: edges with one face
    e = np.sort(np.concatenate((f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]])), axis=1)
    assert (np.unique(e, axis=0, return_counts=True)[1] == 1).any()
    v, f = g20["unref_40_vertices_in"], g20["unref_40_faces_in"]
    assert len(np.unique(f)) == len(v) - 1                              # a vertex no face refers to
    assert int(g20["ico2_keep_target"]) >= len(g20["ico2_keep_faces_in"]) and int(g20["ico1_0_target"]) == 0
    assert len(g20["unref_keep_vertices"]) == len(g20["unref_keep_vertices_in"]) - 1
    assert g20["unref_keep_faces"].tobytes() != g20["unref_keep_faces_in"].tobytes()       # renumbered


@pytest.mark.parametrize("name", NAMES)
def test_sequential_emulator_equals_the_reference(g20, name):
    v, f, target, aggr, ov, of = _case(g20, name)
    ev, ef = simplify_emu.simplify(v, f, target, aggr)
    assert ev.dtype == np.float64 and ef.dtype == np.int32
    assert ev.shape == ov.shape and ef.shape == of.shape
    assert ef.tobytes() == of.tobytes()
    assert ev.tobytes() == ov.tobytes()


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("name", NAMES)
def test_round_emulator_equals_the_reference(g20, name, order):
    v, f, target, aggr, ov, of = _case(g20, name)
    stats = {}
    rv, rf = simplify_emu.simplify_rounds(v, f, target, aggr, order=order, stats=stats)
    assert rf.tobytes() == of.tobytes() and rv.tobytes() == ov.tobytes()
    assert stats["max_rounds_over_candidates"] <= 0                    # a pass never needs more rounds than it has candidates
    assert [stats["iterations"], stats["rounds"], stats["repeats"], stats["longest_pass"]] == g20[name + "_stats"].tolist()


def test_round_emulator_with_the_smallest_reference_lists(g20):
    """The overflow path: with the smallest appended room the lists are rebuilt from the live faces, the result is the same."""
    v, f, target, aggr, ov, of = _case(g20, "ico2_32")
    stats = {}
    rv, rf = simplify_emu.simplify_rounds(v, f, target, aggr, ref_extra=_capi.SIMPLIFY_MIN_REF_EXTRA, stats=stats)
    assert rf.tobytes() == of.tobytes() and rv.tobytes() == ov.tobytes()
    assert stats["rebuilds"] >= 1


def test_simplify_symbols_are_exported_and_reject_bad_arguments():
    lib = _capi.lib()
    for name in ("giga_simplify_workspace_bytes", "giga_mesh_simplify"):
        assert name in _capi.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    assert "#define GIGA_SIMPLIFY_MIN_REF_EXTRA %d" % _capi.SIMPLIFY_MIN_REF_EXTRA in hdr
    size = lib.giga_simplify_workspace_bytes
    ws = size(1, 100, 200, -1)
    # per vertex p, q and their copies (2 x 13 doubles), per face err (3 x 4 doubles) and n (2 x 3), the lists and their copy
    assert ws >= 100 * 26 * 8 + 200 * 18 * 8 + 2 * (6 * 200 + 64) * 4 and ws % 256 == 0
    assert size(1, 100, 200, 64) < ws < size(2, 200, 400, -1)
    assert size(1, 0, 0, -1) > 0                                       # an empty batch entry is a valid call
    assert size(0, 100, 200, -1) == 0 and size(1, -1, 200, -1) == 0 and size(1, 100, -1, -1) == 0
    assert size(1, 100, 200, _capi.SIMPLIFY_MIN_REF_EXTRA - 1) == 0 and size(_capi.MAX_SCENES + 1, 100, 200, -1) == 0
    assert size(1, 100, 0x10000000, -1) == 0
    host = (ctypes.c_int32 * 16)()
    fake = ctypes.addressof(host)                       # never dereferenced: every check precedes the first HIP call
    off = (ctypes.c_int32 * 2)(0, 4)
    tgt = (ctypes.c_int32 * 1)(2)

    def call(**k):
        return lib.giga_mesh_simplify(k.get("v", fake), k.get("f64", 0), k.get("voff", off), k.get("f", fake), k.get("foff", off),
                                      k.get("targets", tgt), k.get("B", 1), k.get("aggr", 5.0), k.get("extra", -1),
                                      k.get("ov", fake), k.get("of", fake), k.get("oc", fake), None, k.get("ws", fake),
                                      k.get("wsb", 1 << 40), None)
    assert call(B=0) == 0
    assert call(B=-1) == -1 and call(B=_capi.MAX_SCENES + 1) == -7
    assert call(v=None) == -1 and call(f=None) == -1 and call(ws=None) == -1 and call(targets=None) == -1
    assert call(voff=None) == -1 and call(foff=None) == -1
    assert call(voff=(ctypes.c_int32 * 2)(1, 4)) == -1 and call(foff=(ctypes.c_int32 * 2)(0, -1)) == -1
    assert call(targets=(ctypes.c_int32 * 1)(-1)) == -1
    assert call(aggr=float("nan")) == -1 and call(f64=2) == -1
    assert call(extra=_capi.SIMPLIFY_MIN_REF_EXTRA - 1) == -1
    assert call(ov=None) == -6 and call(of=None) == -6 and call(oc=None) == -6
    assert call(wsb=size(1, 4, 4, -1) - 1) == -4
    assert b"vertex range" in lib.giga_strerror(-11) and b"round bound" in lib.giga_strerror(-12)


def test_simplify_mesh_has_no_cpu_path():
    from giga_amd.mesh import simplify_mesh
    with pytest.raises(_capi.GigaHipError):
        simplify_mesh(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int32), 2)
    with pytest.raises(ValueError):
        simplify_mesh(torch.zeros(4, 2), torch.zeros(4, 3, dtype=torch.int32), 2)


def test_generator_stores_simplify_nfaces_and_keeps_the_pinned_errors():
    from giga_amd.generation import Generator3D
    gen = Generator3D(None, simplify_nfaces=1000)
    assert gen.simplify_nfaces == 1000 and gen.mesh_options["simplify_nfaces"] == 1000 and gen.refinement_step == 0
    assert Generator3D(None).simplify_nfaces is None
    with pytest.raises(NotImplementedError, match="runs only on a HIP device"):
        Generator3D(None, device=torch.device("cpu"), simplify_nfaces=1000)
    with pytest.raises(NotImplementedError, match="refine_mesh"):      # the combination stays unbuilt; the message names the route
        Generator3D(None, refinement_step=1, simplify_nfaces=100)
    with pytest.raises(ValueError):
        Generator3D(None, simplify_nfaces=-1)
