"""CPU tests of the mesh evaluation: the float64 restatements of tests/eval_emu.py reproduce the reference's recorded results
(tests/golden/g17_eval.npz, tools/make_eval_goldens.py) and, where the reference checkout is present, the live reference;
every new C ABI entry rejects bad arguments before it touches a device; the host-side pieces of giga_amd.eval."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_emu  # noqa: E402


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_mesh.npz")


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_eval.npz")


@pytest.fixture(scope="module", params=list(eval_emu.CASES))
def case(request, g16, g17):
    name = request.param
    inp = eval_emu.case_inputs(g16, name, int(g17[name + "_seed"]))
    assert np.array_equal(eval_emu.checksum(inp), g17[name + "_checksum"]), "regenerated inputs differ from the fixture's"
    return name, inp


def test_fixture_records_the_shares_the_tests_rely_on(g17):
    for name in eval_emu.CASES:
        assert float(g17[name + "_near_tie_share"]) <= 1e-3
        assert int(g17[name + "_near_threshold"]) == 0            # so the F-score counts are exact
        assert float(g17[name + "_kdtree_vs_float64"]) <= 1e-6


def test_restatement_reproduces_the_reference_neighbours(case, g17):
    name, inp = case
    for tag, src, tgt in (("comp", inp["tgt"], inp["pred"]), ("acc", inp["pred"], inp["tgt"])):
        d, i, second = eval_emu.nn_brute(src, tgt)
        ref = g17["%s_%s_dist" % (name, tag)].astype(np.float64)
        assert (np.abs(ref - d) <= 1e-6 * d).all()
        clear = ~eval_emu.near_tie(d, second)
        assert clear.mean() >= 0.999
        assert np.array_equal(i[clear], g17["%s_%s_idx" % (name, tag)].astype(np.int64)[clear])
    dots = eval_emu.normal_dots(g17[name + "_acc_idx"].astype(np.int64), inp["n_pred"], inp["n_tgt"])
    assert np.abs(dots - g17[name + "_acc_dot"]).max() <= 1e-6


def test_restatement_reproduces_the_reference_metrics(case, g17):
    name, inp = case
    want = dict(zip((str(k) for k in g17[name + "_metric_keys"]), g17[name + "_metrics"]))
    eval_emu.assert_metrics(eval_emu.eval_pointcloud(inp["pred"], inp["tgt"], inp["n_pred"], inp["n_tgt"]), want, name)


@pytest.mark.parametrize("resolution", [512, 128])
def test_restatement_reproduces_the_reference_containment(case, g17, resolution):
    name, inp = case
    got = eval_emu.mesh_contains(inp["v"], inp["f"], inp["pts"], resolution)
    want = np.unpackbits(g17["%s_contains_%d" % (name, resolution)])[:len(got)].astype(bool)
    assert np.array_equal(got, want)
    if resolution == 512:
        assert abs(float(eval_emu.compute_iou(got, inp["occ_tgt"])) - float(g17[name + "_iou"])) <= 1e-12


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32_10"""
    assert [int(x) for x in eval_emu.philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    m = 0xffffffff
    assert [int(x) for x in eval_emu.philox4x32_10(m, m, m, m, m, m)] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    got = eval_emu.philox4x32_10(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0)
    assert [int(x) for x in got] == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_sampler_restatement_properties(g16):
    v, f = eval_emu.fixture_mesh(g16, "A")
    f = np.concatenate([f, [[0, 0, 1]]])                            # a face without area
    s = eval_emu.sample_surface(v, f, 5000, seed=11)
    assert s["face"].max() < len(f) - 1 and (eval_emu.face_areas(v, f)[s["face"]] > 0).all()
    assert all(((r >= 0) & (r < 1)).all() for r in s["r"])
    assert len(eval_emu.sample_surface(v, np.zeros((0, 3), np.int64), 10, 0)["points"]) == 0
    assert len(eval_emu.sample_surface(v, np.array([[0, 0, 1]]), 10, 0)["points"]) == 0


@pytest.mark.reference
def test_restatement_against_the_live_reference(g16, tmp_path):
    from oracle import ref_bootstrap
    if not ref_bootstrap.reference_available():
        pytest.skip("reference checkout not present")
    import types
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_eval_goldens
    ref_eval = make_eval_goldens.reference_eval(str(tmp_path))
    v, f = eval_emu.fixture_mesh(g16, "A")
    tv, _ = eval_emu.target_mesh(v, f)
    pred, n_pred = eval_emu.numpy_cloud(v, f, 1500, 5)
    tgt, n_tgt = eval_emu.numpy_cloud(tv, f, 1700, 6)
    dist, dots = ref_eval.distance_p2p(pred, n_pred, tgt, n_tgt)
    d, i, second = eval_emu.nn_brute(pred, tgt)
    assert (np.abs(dist - d) <= 1e-6 * d).all()
    assert np.abs(eval_emu.normal_dots(i, n_pred, n_tgt) - dots).max() <= 1e-5
    eval_emu.assert_metrics(eval_emu.eval_pointcloud(pred, tgt, n_pred, n_tgt),
                            ref_eval.MeshEvaluator().eval_pointcloud(pred, tgt, n_pred, n_tgt), "live")
    pts = eval_emu.iou_points(9)[:4000]
    mesh = types.SimpleNamespace(vertices=v, faces=f)
    for res in (512, 64):
        assert np.array_equal(ref_eval.check_mesh_contains(mesh, pts, hash_resolution=res), eval_emu.mesh_contains(v, f, pts, res))


# ---------------------------------------------------------------------------------------------------------------- the C ABI
def _offs(*xs):
    return (ctypes.c_int32 * len(xs))(*xs)


_BUF = (ctypes.c_double * 64)()
A = ctypes.cast(_BUF, ctypes.c_void_p)
NUL = ctypes.c_void_p(0)
BIG = 1 << 30


def _nn(src=A, so=(0, 4), tgt=A, to=(0, 4), B=1, dist=A, idx=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_nn_query(src, _offs(*so) if so is not None else NUL, tgt, _offs(*to) if to is not None else NUL, B, dist,
                                     idx, ws, ws_bytes, NUL)


def _sample(v=A, vo=(0, 4), t=A, fo=(0, 2), B=1, n=8, first_scene=0, points=A, face=A, normals=A, counts=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_mesh_sample(v, _offs(*vo) if vo is not None else NUL, t, _offs(*fo) if fo is not None else NUL, B, n, 0, first_scene,
                                        points, face, normals, counts, ws, ws_bytes, NUL)


def _contains(v=A, vo=(0, 4), t=A, fo=(0, 2), p=A, po=(0, 5), B=1, resolution=512, inside=A, ws=A, ws_bytes=BIG):
    return _capi.lib().giga_mesh_contains(v, _offs(*vo) if vo is not None else NUL, t, _offs(*fo) if fo is not None else NUL, p,
                                          _offs(*po) if po is not None else NUL, B, resolution, inside, ws, ws_bytes, NUL)


def test_new_entries_are_exported():
    L = _capi.lib()
    for name in ("giga_nn_query", "giga_nn_query_workspace_bytes", "giga_mesh_sample", "giga_mesh_sample_workspace_bytes",
                 "giga_mesh_contains", "giga_mesh_contains_workspace_bytes"):
        assert hasattr(L, name) and name in _capi.EXPORTS
    assert L.giga_abi_version() == 3


BIG_B = dict(B=_capi.MAX_SCENES + 1)


@pytest.mark.parametrize("call, kwargs, code", [
    (_nn, dict(src=NUL), -1), (_nn, dict(tgt=NUL), -1), (_nn, dict(ws=NUL), -1), (_nn, dict(so=None), -1), (_nn, dict(to=None), -1),
    (_nn, dict(dist=NUL), -6), (_nn, dict(idx=NUL), -6), (_nn, dict(B=-1), -1), (_nn, BIG_B, -7),
    (_nn, dict(so=(0, -4)), -1), (_nn, dict(B=2, so=(0, 4, 3), to=(0, 1, 2)), -1), (_nn, dict(to=(1, 4)), -1),
    (_nn, dict(ws_bytes=255), -4), (_nn, dict(B=0), 0), (_nn, dict(so=(0, 0)), 0),
    (_sample, dict(v=NUL), -1), (_sample, dict(t=NUL), -1), (_sample, dict(ws=NUL), -1), (_sample, dict(vo=None), -1),
    (_sample, dict(fo=None), -1), (_sample, dict(points=NUL), -6), (_sample, dict(face=NUL), -6), (_sample, dict(normals=NUL), -6),
    (_sample, dict(counts=NUL), -6), (_sample, dict(n=-1), -1), (_sample, dict(first_scene=-1), -1), (_sample, dict(B=-3), -1), (_sample, BIG_B, -7),
    (_sample, dict(B=2, vo=(0, 4, 8), fo=(0, 2, 1)), -1), (_sample, dict(fo=(0, -2)), -1), (_sample, dict(B=3000, n=1 << 20), -1),
    (_sample, dict(ws_bytes=100), -4), (_sample, dict(B=0), 0),
    (_contains, dict(v=NUL), -1), (_contains, dict(t=NUL), -1), (_contains, dict(p=NUL), -1), (_contains, dict(ws=NUL), -1),
    (_contains, dict(vo=None), -1), (_contains, dict(fo=None), -1), (_contains, dict(po=None), -1), (_contains, dict(inside=NUL), -6),
    (_contains, dict(resolution=1), -1), (_contains, dict(resolution=0), -1), (_contains, dict(resolution=1 << 20), -1),
    (_contains, dict(B=-1), -1), (_contains, BIG_B, -7), (_contains, dict(B=2, vo=(0, 4, 8), fo=(0, 2, 4), po=(0, 5, 2)), -1),
    (_contains, dict(po=(0, -5)), -1), (_contains, dict(ws_bytes=511), -4), (_contains, dict(B=0), 0), (_contains, dict(po=(0, 0)), 0),
])
def test_new_entries_reject_invalid_arguments_without_a_device(call, kwargs, code):
    assert call(**kwargs) == code


def test_workspace_sizes():
    L = _capi.lib()
    assert L.giga_nn_query_workspace_bytes(0, 10) == 0 and L.giga_nn_query_workspace_bytes(1, -1) == 0
    assert L.giga_nn_query_workspace_bytes(1, 1000) >= 8000
    assert L.giga_mesh_sample_workspace_bytes(2, 1000) >= 8000 + 16
    assert L.giga_mesh_contains_workspace_bytes(1, 1000, 500) >= 1000 * 88 + 500 * 4
    assert L.giga_mesh_contains_workspace_bytes(_capi.MAX_SCENES + 1, 1, 1) == 0


# -------------------------------------------------------------------------------------------------- giga_amd.eval on the host
def test_compute_iou_and_thresholds_against_the_fixture(case, g17):
    from giga_amd import eval as E
    name, inp = case
    occ = np.unpackbits(g17[name + "_contains_512"])[:len(inp["pts"])].astype(bool)
    assert abs(float(E.compute_iou(occ, inp["occ_tgt"])) - float(g17[name + "_iou"])) <= 1e-12
    assert abs(float(E.compute_iou(occ.astype(np.float32) * 0.7, inp["occ_tgt"])) - float(g17[name + "_iou"])) <= 1e-12
    dist = g17[name + "_acc_dist"]
    got = E.get_threshold_percentage(dist, E.DEFAULT_THRESHOLDS)
    assert got == [float(x) for x in eval_emu.threshold_percentage(dist.astype(np.float64))]
    assert np.array_equal(E.DEFAULT_THRESHOLDS, eval_emu.THRESHOLDS)


def test_empty_inputs_give_the_reference_dictionaries(g17):
    from giga_amd import eval as E
    for keys, values, mine in (("empty_pcl_keys", "empty_pcl_values", E.EMPTY_PCL_DICT),
                               ("empty_normals_keys", "empty_normals_values", E.EMPTY_PCL_DICT_NORMALS)):
        assert sorted(mine) == [str(k) for k in g17[keys]]
        assert [float(mine[k]) for k in sorted(mine)] == [float(x) for x in g17[values]]
    ev = E.MeshEvaluator()
    empty = np.zeros((0, 3), np.float32)
    assert ev.eval_pointcloud(empty, np.zeros((5, 3), np.float32)) == E.EMPTY_PCL_DICT
    both = dict(E.EMPTY_PCL_DICT, **E.EMPTY_PCL_DICT_NORMALS)
    assert ev.eval_pointcloud(empty, np.zeros((5, 3), np.float32), empty, np.zeros((5, 3), np.float32)) == both
    from giga_amd.mesh import Mesh
    out = ev.eval_mesh(Mesh.empty(), np.zeros((5, 3), np.float32), np.zeros((5, 3), np.float32), np.zeros((7, 3), np.float32),
                       np.zeros(7, bool))
    assert out == dict(both, iou=0.)
    occ = ev.eval_occ(Mesh.empty(), np.zeros((7, 3), np.float32), np.zeros(7, bool), ext="_x")
    assert occ["iou_x"] == 0. and np.isnan(occ["precision_x"]) and np.isnan(occ["recall_x"])
    with pytest.raises(NotImplementedError):
        ev.eval_mesh(Mesh.empty(), empty, empty, empty, np.zeros(0, bool), remove_wall=True)


def test_cpu_tensors_raise_giga_error():
    from giga_amd import eval as E
    with pytest.raises(_capi.GigaHipError):
        E.distance_p2p(torch.zeros(4, 3), None, torch.zeros(4, 3), None)
    with pytest.raises(_capi.GigaHipError):
        E.check_mesh_contains((torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)), torch.zeros(4, 3))
    with pytest.raises(_capi.GigaHipError):
        E.sample_surface((torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int32)), 4)
