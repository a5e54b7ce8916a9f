"""GPU tests of the mesh evaluation (csrc/giga_eval.hip through giga_amd.eval): nearest neighbours, metrics, containment and the
surface sampler against the reference's recorded results (tests/golden/g17_eval.npz) and the float64 restatements of
tests/eval_emu.py, never against the code's own output; generate_mesh -> eval_mesh end to end.  Reads only tests/golden/."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import eval as E
from giga_amd import networks, synth, weights
from giga_amd.generation import Generator3D
from giga_amd.mesh import Mesh

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_emu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_mesh.npz")


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_eval.npz")


@pytest.fixture(scope="module")
def cases(g16, g17):
    out = {}
    for name in eval_emu.CASES:
        inp = eval_emu.case_inputs(g16, name, int(g17[name + "_seed"]))
        assert np.array_equal(eval_emu.checksum(inp), g17[name + "_checksum"])
        out[name] = inp
    return out


def _nn(src, tgt):
    d, i, _ = E.nn_query_batch([src], [tgt])
    torch.cuda.synchronize()
    assert d.dtype == torch.float32 and i.dtype == torch.int64
    return d.cpu().numpy(), i.cpu().numpy()


def _check_nn(src, tgt, d, i, what=""):
    """the issue's bounds: every distance within 1e-6 relative of float64; the index the float64 one wherever the second-nearest is
    more than 1e-6 (relative) away, at most 0.1 % excluded; everywhere |src - tgt[idx]| within 1e-6 relative of the minimum"""
    d64, i64, second = eval_emu.nn_brute(src, tgt)
    err = np.abs(d.astype(np.float64) - d64) / np.where(d64 > 0, d64, 1.0)
    print(what, "max relative distance error %.3g" % err.max())
    assert (np.abs(d.astype(np.float64) - d64) <= 1e-6 * d64).all()
    clear = ~eval_emu.near_tie(d64, second)
    assert clear.mean() >= 0.999
    assert np.array_equal(i[clear], i64[clear])
    assert ((i >= 0) & (i < len(tgt))).all()
    own = np.linalg.norm(np.asarray(src, np.float64) - np.asarray(tgt, np.float64)[i], axis=1)
    assert (np.abs(own - d64) <= 1e-6 * d64).all()
    return d64, i64, clear


# -------------------------------------------------------------------------------------------------------- nearest neighbour
@pytest.mark.parametrize("name", list(eval_emu.CASES))
def test_nn_matches_the_reference_and_float64(cases, g17, name):
    inp = cases[name]
    for tag, src, tgt in (("comp", inp["tgt"], inp["pred"]), ("acc", inp["pred"], inp["tgt"])):
        d, i = _nn(src, tgt)
        d64, i64, clear = _check_nn(src, tgt, d, i, name + " " + tag)
        ref_d, ref_i = g17["%s_%s_dist" % (name, tag)].astype(np.float64), g17["%s_%s_idx" % (name, tag)].astype(np.int64)
        assert (np.abs(d - ref_d) <= 2e-6 * d64).all()              # both within 1e-6 of float64
        assert np.array_equal(i[clear], ref_i[clear])
        d2, i2 = _nn(src, tgt)                                      # a second run: the same bytes
        assert d.tobytes() == d2.tobytes() and i.tobytes() == i2.tobytes()


@pytest.mark.parametrize("ns, nt", [(1, 1), (1, 3001), (2999, 1), (1237, 2501), (300, 50000), (5000, 70001)])
def test_nn_shapes(ns, nt):
    """1 x 1, 1 x N, N x 1, counts that are no multiple of a tile, and two cases whose targets are split over workgroups
    (few source workgroups, 49 and 69 target tiles)"""
    rng = np.random.default_rng(ns * 7 + nt)
    src, tgt = (rng.random((ns, 3)) - 0.5).astype(np.float32), (rng.random((nt, 3)) - 0.5).astype(np.float32)
    d, i = _nn(src, tgt)
    _check_nn(src, tgt, d, i, "%d x %d" % (ns, nt))


def test_nn_without_targets_and_exact_ties():
    rng = np.random.default_rng(3)
    src = (rng.random((700, 3)) - 0.5).astype(np.float32)
    d, i = _nn(src, np.zeros((0, 3), np.float32))
    assert np.isposinf(d).all() and (i == -1).all()
    base = (rng.random((1500, 3)) - 0.5).astype(np.float32)
    tgt = np.concatenate([base, base, base[::-1]])                  # every target three times, across tiles and splits
    d, i = _nn(src, tgt)
    d64, i64, _ = eval_emu.nn_brute(src, tgt)
    assert (i < 1500).all() and np.array_equal(i, i64)              # argmin's first minimum = the lowest index
    d, i = _nn(base[:100], tgt)
    assert (d == 0).all() and np.array_equal(i, np.arange(100))


def test_nn_ragged_batch_equals_single_calls():
    rng = np.random.default_rng(8)
    sizes = [(700, 1300), (1, 5), (2049, 0), (0, 10), (333, 40000)]
    srcs = [(rng.random((a, 3)) - 0.5).astype(np.float32) for a, _ in sizes]
    tgts = [(rng.random((b, 3)) - 0.5).astype(np.float32) for _, b in sizes]
    d, i, so = E.nn_query_batch(srcs, tgts)
    d, i = d.cpu().numpy(), i.cpu().numpy()
    assert so.tolist() == [0, 700, 701, 2750, 2750, 3083]
    for b in range(len(sizes)):
        if sizes[b][0] == 0:
            continue
        sd, si = _nn(srcs[b], tgts[b])
        assert d[so[b]:so[b + 1]].tobytes() == sd.tobytes() and i[so[b]:so[b + 1]].tobytes() == si.tobytes(), b
    assert np.isposinf(d[so[2]:so[3]]).all() and (i[so[2]:so[3]] == -1).all()


# ------------------------------------------------------------------------------------------------------------------ metrics
@pytest.mark.parametrize("name", list(eval_emu.CASES))
def test_eval_pointcloud_matches_the_reference_dictionary(cases, g17, name):
    inp = cases[name]
    want = dict(zip((str(k) for k in g17[name + "_metric_keys"]), g17[name + "_metrics"]))
    got = E.MeshEvaluator().eval_pointcloud(inp["pred"], inp["tgt"], inp["n_pred"], inp["n_tgt"])
    assert sorted(got) == sorted(want)
    eval_emu.assert_metrics(got, want, name)
    dev = E.MeshEvaluator().eval_pointcloud(*(torch.from_numpy(inp[k]).to(DEV) for k in ("pred", "tgt", "n_pred", "n_tgt")))
    assert dev == got                                               # device tensors in, the same numbers out
    dist, dots = E.distance_p2p(inp["pred"], inp["n_pred"], inp["tgt"], inp["n_tgt"])
    assert np.abs(dots.cpu().numpy() - g17[name + "_acc_dot"]).max() <= 1e-5
    dist, dots = E.distance_p2p(inp["pred"], None, inp["tgt"], None)
    assert bool(torch.isnan(dots).all())


# -------------------------------------------------------------------------------------------------------------- containment
@pytest.mark.parametrize("name", list(eval_emu.CASES))
@pytest.mark.parametrize("resolution", [512, 128])
def test_contains_equals_the_reference_bit_for_bit(cases, g17, name, resolution):
    inp = cases[name]
    want = np.unpackbits(g17["%s_contains_%d" % (name, resolution)])[:len(inp["pts"])].astype(bool)
    got = E.check_mesh_contains((inp["v"], inp["f"]), inp["pts"], hash_resolution=resolution).cpu().numpy()
    print(name, resolution, "inside", int(got.sum()), "mismatches", int((got != want).sum()))
    assert np.array_equal(got, want)
    got64 = E.check_mesh_contains(Mesh(inp["v"], inp["f"]), torch.from_numpy(inp["pts"]).to(DEV).double(), resolution).cpu().numpy()
    assert np.array_equal(got64, want)
    if resolution == 512:
        occ = E.MeshEvaluator().eval_occ((inp["v"], inp["f"]), inp["pts"], inp["occ_tgt"])
        assert abs(float(occ["iou"]) - float(g17[name + "_iou"])) <= 1e-12
        both = want & inp["occ_tgt"]
        assert occ["precision"] == both.sum() / want.sum() and occ["recall"] == both.sum() / inp["occ_tgt"].sum()


def test_contains_outside_box_empty_mesh_and_batch(cases):
    a, b = cases["A"], cases["B"]
    far = np.array([[2.0, 0.0, 0.0], [0.0, 0.0, -0.9], [0.28, 0.0, 0.0], [np.nan, 0.0, 0.0]], np.float32)
    got = E.check_mesh_contains((a["v"], a["f"]), far).cpu().numpy()
    assert got.tolist() == eval_emu.mesh_contains(a["v"], a["f"], far).tolist() == [False, False, True, False]
    assert not E.check_mesh_contains(Mesh.empty(), a["pts"][:100]).any()
    meshes = [(a["v"], a["f"]), (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)), (b["v"], b["f"]), (a["v"], a["f"])]
    pts = [a["pts"][:7001], a["pts"][:50], b["pts"], a["pts"][7001:7003]]
    occ, po = E.mesh_contains_batch(meshes, pts, 512)
    occ = occ.cpu().numpy()
    for k, (m, p) in enumerate(zip(meshes, pts)):
        single = E.check_mesh_contains(m, p).cpu().numpy()
        assert np.array_equal(occ[po[k]:po[k + 1]], single), k
    assert np.array_equal(occ[po[2]:po[3]], eval_emu.mesh_contains(b["v"], b["f"], b["pts"]))


# ------------------------------------------------------------------------------------------------------------------ sampler
def _sample(v, f, n, seed, scene=0):
    p, face, nr = E.sample_surface((v, f), n, seed, scene)
    torch.cuda.synchronize()
    return p.cpu().numpy(), face.cpu().numpy(), nr.cpu().numpy()


@pytest.mark.parametrize("name", list(eval_emu.CASES))
def test_sampler_matches_the_restatement(cases, name):
    v, f = cases[name]["v"], cases[name]["f"]
    f = np.concatenate([f[:100], [[5, 5, 9], [7, 7, 7]], f[100:]])              # two faces without area among them
    n, seed = 50000, 0x1234567890abcdef
    p, face, nr = _sample(v, f, n, seed)
    emu = eval_emu.sample_surface(v, f, n, seed)
    assert p.shape == (n, 3) and p.dtype == np.float32 and face.shape == (n,)
    # the face: the restatement's, except where r0 * total sits within 1e-12 * total of a prefix-sum boundary
    differ = face != emu["face"]
    gap = np.abs(emu["cum"][None, :] - emu["x"][differ, None]).min(axis=1) if differ.any() else np.zeros(0)
    print(name, "faces that differ", int(differ.sum()))
    assert differ.mean() <= 1e-3 and (gap <= 1e-12 * emu["total"]).all()
    area = eval_emu.face_areas(v, f)
    assert (area[face] > 0).all() and not np.isin(face, [100, 101]).any()
    # the point: rebuilt in float64 from the kernel's own face and the restatement's uniforms, and on the face
    want_p, want_n = eval_emu.points_on_faces(v, f, face, emu["r"][1], emu["r"][2])
    bound = 4 * 2.0 ** -24 * np.abs(v).max()
    print(name, "points that differ from the restatement's bits", int((p != want_p).any(axis=1).sum()))
    assert np.abs(p.astype(np.float64) - want_p).max() <= bound
    v64 = v.astype(np.float64)
    a, b, c = v64[f[face, 0]], v64[f[face, 1]], v64[f[face, 2]]
    n64 = np.cross(b - a, c - a)
    n64 /= np.linalg.norm(n64, axis=1, keepdims=True)
    assert np.abs(((p.astype(np.float64) - a) * n64).sum(axis=1)).max() <= bound           # in the face's plane
    m = np.stack([b - a, c - a], axis=2)                                                 # barycentric coordinates >= 0, sum <= 1
    uv = np.stack([np.linalg.lstsq(m[k], p[k].astype(np.float64) - a[k], rcond=None)[0] for k in range(0, n, 97)])
    # a displacement of `bound` per coordinate moves (u, v) by at most sqrt(3) bound / (smallest singular value of the edge matrix)
    scale = np.sqrt(3) * bound / np.array([np.linalg.svd(m[k], compute_uv=False)[-1] for k in range(0, n, 97)])
    assert (uv.min(axis=1) >= -scale).all() and (uv.sum(axis=1) <= 1 + scale).all()
    assert np.abs(np.linalg.norm(nr.astype(np.float64), axis=1) - 1).max() <= 2e-7
    assert np.abs(nr - want_n).max() <= 2e-7 and np.abs(nr.astype(np.float64) - n64).max() <= 2e-7


def test_sampler_face_frequencies_follow_the_areas(cases):
    """chi-square on 32 bins of (nearly) equal area at a fixed seed.  With K = 32 bins the statistic has 31 degrees of freedom; its
    1 - 1e-6 quantile is 78.6 (Wilson-Hilferty: 31 (1 - 2/279 + 4.7534 sqrt(2/279))^3 = 78.6; tables give 78.5), used as 79"""
    v, f = cases["A"]["v"], cases["A"]["f"]
    n = 200000
    _, face, _ = _sample(v, f, n, 2024)
    cum = np.cumsum(eval_emu.face_areas(v, f))
    edges = np.searchsorted(cum, cum[-1] * np.arange(1, 32) / 32)
    bins = np.searchsorted(edges, np.arange(len(f)), side="right")
    expected = n * np.bincount(bins, weights=eval_emu.face_areas(v, f), minlength=32) / cum[-1]
    observed = np.bincount(bins[face], minlength=32)
    chi2 = float(((observed - expected) ** 2 / expected).sum())
    print("chi-square", chi2)
    assert chi2 <= 79.0


def test_sampler_seeds_batches_and_empty_meshes(cases):
    a, b = cases["A"], cases["B"]
    p0, f0, n0 = _sample(a["v"], a["f"], 10000, 5)
    p1, f1, n1 = _sample(a["v"], a["f"], 10000, 5)
    assert p0.tobytes() == p1.tobytes() and f0.tobytes() == f1.tobytes() and n0.tobytes() == n1.tobytes()
    p2, _, _ = _sample(a["v"], a["f"], 10000, 6)
    assert not np.array_equal(p0, p2)
    p3, _, _ = _sample(a["v"], a["f"], 777, 5)                      # the first 777 of the 10 000: no dependence on launch geometry
    assert p3.tobytes() == p0[:777].tobytes()
    flat = (a["v"][:3], np.array([[0, 0, 1]]))
    meshes = [(a["v"], a["f"]), Mesh.empty(), (b["v"], b["f"]), flat, (a["v"], a["f"])]
    p, face, nr, counts = E.sample_surface_batch(meshes, 4000, seed=5)
    assert counts.tolist() == [4000, 0, 4000, 0, 4000]
    for k in (0, 2, 4):
        sp, sf, sn = _sample(*E.ragged.mesh_parts(meshes[k]), 4000, 5, scene=k)
        assert p[k].cpu().numpy().tobytes() == sp.tobytes() and np.array_equal(face[k].cpu().numpy(), sf), k
        assert nr[k].cpu().numpy().tobytes() == sn.tobytes(), k
    assert not np.array_equal(p[0].cpu().numpy(), p[4].cpu().numpy())       # the same mesh as another scene: other samples
    assert p0[:4000].tobytes() == p[0].cpu().numpy().tobytes()
    for m in (Mesh.empty(), flat):
        assert [len(x) for x in E.sample_surface(m, 100)] == [0, 0, 0]


# --------------------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def net():
    n = networks.get_network("giga")
    n.load_state_dict(weights.make_state_dict(7))
    return n.to(DEV).eval()


def _restated_eval(mesh, n_points, seed, tgt, n_tgt, pts, occ_tgt):
    """eval_mesh restated on the host copy of the mesh: the restatement's samples, float64 neighbours, containment over all faces"""
    s = eval_emu.sample_surface(mesh.vertices, mesh.faces, n_points, seed)
    out = eval_emu.eval_pointcloud(s["points"], tgt, s["normals"], n_tgt)
    out["iou"] = eval_emu.compute_iou(eval_emu.mesh_contains(mesh.vertices, mesh.faces, pts), occ_tgt)
    return out


def test_generate_mesh_then_eval_mesh(net, g16, cases):
    gen = Generator3D(net, device=DEV, threshold=float(g16["B_threshold"]), resolution0=32, upsampling_steps=0, padding=0.0)
    x = torch.from_numpy(synth.tsdf_batch(70, 1)).to(DEV)
    mesh = gen.generate_mesh({"inputs": x})
    mesh = mesh[0] if isinstance(mesh, (tuple, list)) else mesh
    assert len(mesh.vertices) > 1000
    b = cases["B"]
    ev = E.MeshEvaluator(n_points=6000, seed=3)
    got = ev.eval_mesh(mesh, b["tgt"], b["n_tgt"], b["pts"], b["occ_tgt"])
    want = _restated_eval(mesh, 6000, 3, b["tgt"], b["n_tgt"], b["pts"], b["occ_tgt"])
    eval_emu.assert_metrics(got, want, "end to end")
    assert abs(float(got["iou"]) - float(want["iou"])) <= 1e-12
    on_device = (torch.from_numpy(mesh.vertices).to(DEV), torch.from_numpy(mesh.faces).to(DEV))
    assert ev.eval_mesh(on_device, b["tgt"], b["n_tgt"], b["pts"], b["occ_tgt"]) == got


def test_eval_meshes_equals_single_calls(cases):
    a, b = cases["A"], cases["B"]
    meshes = [Mesh(a["v"], a["f"]), Mesh.empty(), Mesh(b["v"], b["f"])]
    tgts, nts = [a["tgt"][:5000], a["tgt"][:10], b["tgt"]], [a["n_tgt"][:5000], a["n_tgt"][:10], b["n_tgt"]]
    pts, occ = [a["pts"][:3000], a["pts"][:10], b["pts"][:4000]], [a["occ_tgt"][:3000], a["occ_tgt"][:10], b["occ_tgt"][:4000]]
    ev = E.MeshEvaluator(n_points=4000, seed=1)
    batch = ev.eval_meshes(meshes, tgts, nts, pts, occ)
    for k in range(3):
        single = ev.eval_mesh(meshes[k], tgts[k], nts[k], pts[k], occ[k])
        assert batch[k].keys() == single.keys()
        for key in single:
            assert np.array_equal(np.float64(batch[k][key]), np.float64(single[key])), (k, key)
    assert batch[1]["iou"] == 0. and batch[1]["empty"] is True
