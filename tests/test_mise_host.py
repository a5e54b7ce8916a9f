"""CPU tests of MISE: the dict / set restatement of the reference's libmise (tests/mise_emu.py) against the reference's own
compiled libmise (tests/golden/g19_mise.npz, written by tools/make_mise_goldens.py), the C ABI's argument checks and workspace
size, and the host-side contracts of `giga_amd.mise` and `Generator3D(mise=True)`."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mise_emu  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ["sphere43", "sphere42", "slab43", "ball43", "sphere32", "sphere41", "positive22", "negative22", "plane42", "faces42"]


def fixture_case(g19, name):
    """(field, resolution0, depth, threshold, list of per-round sorted index arrays, dense grid) of one fixture case."""
    res0, depth = (int(x) for x in g19[name + "_setup"])
    sizes = g19[name + "_sizes"].tolist()
    rounds = np.split(g19[name + "_rounds"], np.cumsum(sizes)[:-1]) if sizes else []
    return g19[name + "_field"], res0, depth, float(g19[name + "_threshold"]), rounds, g19[name + "_dense"]


def test_the_fixture_holds_the_cases_it_is_meant_to(golden):
    g19 = golden("g19_mise.npz")
    assert list(g19["names"]) == CASES
    sizes = {n: g19[n + "_sizes"].tolist() for n in CASES}
    assert sizes["sphere42"] == [125, 344, 1232]                            # libmise's round sizes on these fields
    assert sizes["slab43"] == [125, 344, 1505, 6116, 3376] and len(sizes["slab43"]) > 3 + 1
    assert sizes["ball43"] == [125] and not (g19["ball43_dense"] >= 0).any() and (g19["ball43_field"] >= 0).any()
    assert sizes["positive22"] == [27] and sizes["negative22"] == [27]
    assert int(g19["sphere32_setup"][0]) == 3 and int(g19["sphere41_setup"][1]) == 1
    plane = g19["plane42_field"]
    assert (plane == np.round(plane)).all() and (plane[8] == float(g19["plane42_threshold"])).all()
    f = g19["faces42_field"]
    for face in (f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1]):  # the surface cuts all six boundary faces
        assert (face > 0).any() and (face < 0).any()
    for n in CASES:
        assert g19[n + "_field"].dtype == np.float32 and g19[n + "_dense"].dtype == np.float32 and g19[n + "_rounds"].dtype == np.int32


@pytest.mark.parametrize("name", CASES)
def test_emulator_reproduces_libmise(golden, name):
    field, res0, depth, thr, rounds, dense = fixture_case(golden("g19_mise.npz"), name)
    got_rounds, got_dense = mise_emu.run(field, res0, depth, thr)
    assert [len(r) for r in got_rounds] == [len(r) for r in rounds]
    for k, (a, b) in enumerate(zip(got_rounds, rounds)):
        assert a.dtype == np.int32 and np.array_equal(a, b), k
    assert got_dense.dtype == np.float32 and got_dense.tobytes() == dense.tobytes()


def test_sphere_cells_of_to_dense_are_those_of_the_dense_field(golden):
    """The surface-crossing cells of to_dense() are exactly those of the field it sampled (sphere, resolution0 4, depth 3)."""
    field, _, _, thr, _, dense = fixture_case(golden("g19_mise.npz"), "sphere43")

    def crossing(g):
        inside = g >= thr
        n = g.shape[0] - 1
        corners = sum(inside[a:a + n, b:b + n, c:c + n].astype(np.int64) for a in (0, 1) for b in (0, 1) for c in (0, 1))
        return (corners > 0) & (corners < 8)

    assert crossing(field).sum() > 0 and np.array_equal(crossing(field), crossing(dense))


def _workspace_bytes(B, res0, depth):
    """The layout of csrc/giga_mise.hip: counts, workgroup sums, the activity byte per 1024 samples, state, tree, values, each
    rounded up to 256 bytes."""
    up = lambda x: (x + 255) // 256 * 256
    n3 = ((res0 << depth) + 1) ** 3
    words = (n3 + 3) // 4
    nblk = (words + 255) // 256
    tree = sum(((res0 << l) ** 3 + 3) // 4 * 4 for l in range(depth))
    return up(4 * B) + up(4 * B * nblk) + up(B * nblk) + up(4 * B * words) + up(B * tree) + up(4 * B * n3)


def test_mise_symbols_constants_and_workspace():
    lib = _capi.lib()
    names = ("giga_mise_workspace_bytes", "giga_mise_init", "giga_mise_count", "giga_mise_emit", "giga_mise_update", "giga_mise_to_dense")
    for name in names:
        assert name in _capi.EXPORTS and hasattr(lib, name)
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    for name in names:
        assert name + "(" in hdr
    assert "#define GIGA_MISE_MAX_N %d" % _capi.MISE_MAX_N in hdr
    assert "#define GIGA_MESH_MAX_N %d" % _capi.MESH_MAX_N in hdr
    assert _capi.MESH_MAX_N >= _capi.MISE_MAX_N >= 513               # every MISE grid can be meshed
    assert lib.giga_abi_version() == 3                               # additive entry points: the version stays
    for B, res0, depth in ((1, 4, 3), (3, 3, 2), (1, 16, 3), (2, 4, 1), (1, 32, 4), (1, 1, 1)):
        assert lib.giga_mise_workspace_bytes(B, res0, depth) == _workspace_bytes(B, res0, depth), (B, res0, depth)
    wsb = lib.giga_mise_workspace_bytes
    assert wsb(0, 4, 3) == 0 and wsb(-1, 4, 3) == 0 and wsb(1, 0, 3) == 0 and wsb(1, 4, 0) == 0 and wsb(1, 4, -1) == 0
    assert wsb(1, 32, 4) > 0 and wsb(1, 33, 4) == 0 and wsb(1, 32, 5) == 0 and wsb(1, 1, 31) == 0 and wsb(1, 1 << 30, 2) == 0
    assert wsb(15, 32, 4) > 0 and wsb(16, 32, 4) == 0               # 16 x 513^3 >= 2^31 samples
    assert wsb(_capi.MAX_SCENES + 1, 1, 1) == 0


def test_mise_entry_points_reject_bad_arguments_before_any_hip_call():
    lib = _capi.lib()
    host = (ctypes.c_float * 16)()
    fake = ctypes.addressof(host)                       # never dereferenced: every check precedes the first launch
    big = 1 << 40
    need = lib.giga_mise_workspace_bytes(1, 4, 2)
    init = lambda **k: lib.giga_mise_init(k.get("B", 1), k.get("r", 4), k.get("d", 2), k.get("ws", fake), k.get("wsb", big), None)
    count = lambda **k: lib.giga_mise_count(k.get("B", 1), k.get("r", 4), k.get("d", 2), k.get("ws", fake), k.get("wsb", big),
                                            k.get("counts", fake), None)
    emit = lambda **k: lib.giga_mise_emit(k.get("B", 1), k.get("r", 4), k.get("d", 2), k.get("ws", fake), k.get("wsb", big),
                                          k.get("q", fake), k.get("cap", 4), None, k.get("lin", fake), k.get("pts", fake), None)
    update = lambda **k: lib.giga_mise_update(k.get("v", fake), k.get("q", fake), k.get("cap", 4), k.get("B", 1), k.get("r", 4),
                                              k.get("d", 2), k.get("thr", 0.0), k.get("ws", fake), k.get("wsb", big), None)
    dense = lambda **k: lib.giga_mise_to_dense(k.get("B", 1), k.get("r", 4), k.get("d", 2), k.get("ws", fake), k.get("wsb", big),
                                               k.get("grid", fake), None)
    for fn in (init, count, emit, update, dense):
        assert fn(B=0) == 0
        assert fn(B=-1) == -1 and fn(r=0) == -1 and fn(d=0) == -1 and fn(d=31) == -1 and fn(r=33, d=4) == -1
        assert fn(B=16, r=32, d=4) == -1                             # 2^31 samples or more in one call
        assert fn(B=_capi.MAX_SCENES + 1) == -7
        assert fn(ws=None) == -1
        assert fn(wsb=need - 1) == -4
    assert count(counts=None) == -1
    assert emit(q=None) == -6
    assert emit(lin=None) == -1 and emit(cap=1 << 31) == -1
    assert update(v=None) == -1 and update(q=None) == -1 and update(thr=float("nan")) == -1 and update(cap=1 << 31) == -1
    assert dense(grid=None) == -1


def test_lin_table_is_the_float64_arithmetic_of_the_reference():
    from giga_amd.generation import Generator3D
    from giga_amd.mise import lin_table
    for res0, steps, padding in ((16, 3, 0.1), (4, 3, 0.1), (3, 2, 0.0), (32, 4, 0.1), (5, 1, 0.25)):
        gen = Generator3D(None, device=torch.device("cpu"), resolution0=res0, upsampling_steps=steps, padding=padding, mise=True)
        R = res0 * 2 ** steps
        idx = np.arange(R + 1, dtype=np.int64)
        pointsf = idx / R                                            # generation.py:132-135, float64 throughout
        want = ((1 + padding) * (pointsf - 0.5)).astype(np.float32)
        lin = gen.mise_lin()
        assert lin.dtype == np.float32 and lin.shape == (gen.grid_resolution(),) and lin.tobytes() == want.tobytes()
        assert lin.tobytes() == lin_table(R, 1 + padding).tobytes()
        assert lin[0] == np.float32(-(1 + padding) / 2) and lin[-1] == np.float32((1 + padding) / 2) and lin[R // 2] == 0


def test_generator_takes_mise_and_there_is_no_cpu_path():
    from giga_amd.generation import Generator3D
    from giga_amd.mise import MISE, mise_grid
    gen = Generator3D(None, device=torch.device("cpu"), mise=True)
    assert gen.mise is True and gen.grid_resolution() == 129
    assert Generator3D(None, device=torch.device("cpu")).mise is False          # the default stays the dense grid
    assert abs(Generator3D(None, device=torch.device("cpu"), threshold=0.6, mise=True)._iso() - (np.log(0.6) - np.log(0.4))) < 1e-15
    with pytest.raises(_capi.GigaHipError):
        MISE(4, 2, 0.0, device="cpu")
    with pytest.raises(_capi.GigaHipError):
        mise_grid(lambda q, p: torch.zeros(q.shape), 4, 2, 0.0, device=torch.device("cpu"))
