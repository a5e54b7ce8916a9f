"""GPU tests of MISE on the device: the giga_mise_* kernels (csrc/giga_mise.hip) through `giga_amd.mise` on the fixtures of
tests/golden/g19_mise.npz (the reference's libmise, tools/make_mise_goldens.py) with a lookup into the uploaded field as the
value function, so that the device and libmise see identical values; then `Generator3D(mise=True)` end to end with the real
decoder in the loop against the emulator of tests/mise_emu.py.  Reads only tests/golden/."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, networks, synth, weights
from giga_amd.generation import Generator3D
from giga_amd.mise import MISE, mise_grid

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mise_emu  # noqa: E402
from test_mise_host import CASES, fixture_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# tests/test_gpu_parity.py::test_model_forward_g2 holds the fp32 occupancy logits (`tsdf`) to tol * 2 with tol = 1e-4
TAU = 2e-4


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_mise.npz")


def _lookup(fields):
    """value_fn over uploaded fields (B, N^3): the value at every queried index (columns past a scene's count hold index 0)."""
    flat = fields.reshape(fields.shape[0], -1)
    return lambda q, pts: flat.gather(1, q.long().clamp(0, flat.shape[1] - 1))


def _run(fields, res0, depth, thr):
    """(per-round list of per-scene sorted index arrays, dense grids as numpy) of a device run on `fields` (B,N,N,N) numpy."""
    dev_fields = torch.from_numpy(np.ascontiguousarray(fields)).to(DEV)
    rounds, stats = [], {}
    dense = mise_grid(_lookup(dev_fields), res0, depth, thr, batch=len(fields), device=DEV, stats=stats, rounds=rounds)
    torch.cuda.synchronize()
    per_round = []
    for q, counts in rounds:
        q = q.cpu().numpy()
        assert q.dtype == np.int32 and q.shape == (len(fields), max(counts))
        per_round.append([q[b, :counts[b]] for b in range(len(fields))])
    assert stats["mise rounds"] == len(rounds) and stats["mise points"] == sum(sum(c) for _, c in rounds)
    return per_round, dense.cpu().numpy()


@pytest.mark.parametrize("name", CASES)
def test_rounds_and_dense_grid_equal_libmise(g19, name):
    field, res0, depth, thr, want_rounds, want_dense = fixture_case(g19, name)
    rounds, dense = _run(field[None], res0, depth, thr)
    print(name, "round sizes", [len(r[0]) for r in rounds])
    assert [len(r[0]) for r in rounds] == [len(r) for r in want_rounds]
    for k, (got, want) in enumerate(zip(rounds, want_rounds)):
        assert np.array_equal(got[0], want), k                       # ascending linear index = the fixture's sorted set
    assert dense.dtype == np.float32 and dense.shape == (1,) + want_dense.shape and not np.isnan(dense).any()
    assert dense[0].tobytes() == want_dense.tobytes()
    rounds2, dense2 = _run(field[None], res0, depth, thr)            # a second run: the same bytes
    assert all(a[0].tobytes() == b[0].tobytes() for a, b in zip(rounds, rounds2)) and dense.tobytes() == dense2.tobytes()


def test_more_than_1024_workgroups_per_scene_against_the_emulator():
    """resolution0 13, depth 3: 105^3 samples are 1131 runs of 1024 (the fixture's largest lattice, 33^3, has 36), so the scan of a
    scene's workgroup sums takes a second round of 1024.  13 is the smallest resolution0 that gets there at the generator's default
    depth.  A small ball about the last lattice plane along x: the queries of every round reach into the runs past the 1024th."""
    res0, depth = 13, 3
    N = (res0 << depth) + 1
    assert -(-(-(-N ** 3 // 4)) // 256) == 1131
    i, j, k = np.meshgrid(*[np.arange(N, dtype=np.float64)] * 3, indexing="ij")
    field = (9.5 - np.sqrt((i - 100) ** 2 + (j - 52.3) ** 2 + (k - 51.8) ** 2)).astype(np.float32)
    want_rounds, want_dense = mise_emu.run(field, res0, depth, 0.0)
    assert len(want_rounds) == depth + 1 and all(r[-1] >= 1024 * 1024 for r in want_rounds)
    rounds, dense = _run(field[None], res0, depth, 0.0)
    assert [len(r[0]) for r in rounds] == [len(r) for r in want_rounds]
    for k, (got, want) in enumerate(zip(rounds, want_rounds)):
        assert np.array_equal(got[0], want), k
    assert dense[0].tobytes() == want_dense.tobytes()


def test_three_scenes_with_different_round_counts_equal_single_runs(g19):
    names = ["sphere43", "slab43", "ball43"]                         # 4, 5 and 1 rounds on the same 33^3 lattice, threshold 0
    cases = [fixture_case(g19, n) for n in names]
    assert len({c[1:4] for c in cases}) == 1 and len({len(c[4]) for c in cases}) == 3
    _, res0, depth, thr = cases[0][:4]
    rounds, dense = _run(np.stack([c[0] for c in cases]), res0, depth, thr)
    assert len(rounds) == max(len(c[4]) for c in cases)
    for b, (name, case) in enumerate(zip(names, cases)):
        single_rounds, single_dense = _run(case[0][None], res0, depth, thr)
        for k, r in enumerate(rounds):
            want = single_rounds[k][0] if k < len(single_rounds) else np.zeros(0, np.int32)
            assert r[b].tobytes() == want.tobytes(), (name, k)
            assert np.array_equal(want, case[4][k] if k < len(case[4]) else want), (name, k)
        assert dense[b].tobytes() == single_dense[0].tobytes() == case[5].tobytes(), name


def test_short_query_capacity_is_reported_and_guards_stay(g19):
    field, res0, depth, thr, want_rounds, _ = fixture_case(g19, "sphere42")
    fields = torch.from_numpy(np.stack([field, -field])).to(DEV)    # two scenes: the second sees the complement
    m = MISE(res0, depth, thr, batch=2, device=DEV)
    m.update(_lookup(fields)(m.query(), None))                       # round 1, so that the lists are no longer a regular lattice
    full = m.query().clone()
    counts = list(m.counts)
    assert counts[0] == len(want_rounds[1]) and min(counts) > 8
    L, ws = _capi.lib(), m._ws
    cnt = torch.zeros(2, dtype=torch.int32, device=DEV)
    GUARD = 64
    for short in (0, 1, 5):
        cap = max(counts) - short
        buf = torch.full((2 * cap + GUARD,), -777, dtype=torch.int32, device=DEV)
        sf = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        _capi.check(L.giga_mise_count(2, res0, depth, _capi.ptr(ws), ws.numel(), _capi.ptr(cnt), _capi.stream_ptr(DEV)), "count")
        _capi.check(L.giga_mise_emit(2, res0, depth, _capi.ptr(ws), ws.numel(), _capi.ptr(buf), cap, _capi.ptr(sf), None, None,
                                     _capi.stream_ptr(DEV)), "emit")
        torch.cuda.synchronize()
        assert cnt.tolist() == counts                                # the counts are the full lengths, whatever the capacity
        assert sf.tolist() == [max(c - cap, 0) for c in counts]
        assert bool((buf[2 * cap:] == -777).all())
        for b in range(2):
            kept = min(counts[b], cap)
            assert torch.equal(buf[b * cap:b * cap + kept], full[b, :kept])
            assert bool((buf[b * cap + kept:(b + 1) * cap] == -777).all())     # nothing past a scene's own list either


# ---- end to end: the real decoder in the loop ------------------------------------------------------------------------------
SCENE, THRESHOLD, BALL_THRESHOLD = 40, 0.7815, 0.8428       # chosen with the CPU oracle: see `e2e` below


@pytest.fixture(scope="module")
def net():
    n = networks.get_network("giga")
    n.load_state_dict(weights.make_state_dict(7))
    n = n.to(DEV).eval()
    n.set_precision("fp32")
    return n


@pytest.fixture(scope="module")
def e2e(net):
    """Weight seed 7, synth scene 40, resolution0 4, three upsampling steps (33^3), padding 0.1; the full lattice decoded once on
    points built from the same per-axis table.  On the CPU oracle's logits of this lattice the nearest value to
    log(0.7815 / 0.2185) = 1.27443 is 2.9e-3 away (a gap of 5.9e-3 between two neighbours of the sorted values), and at
    threshold 0.8428 (1.67921, 3.6e-2 from the nearest value) one sample, which is no coarse lattice point, lies above."""
    gen = Generator3D(net, device=DEV, threshold=THRESHOLD, resolution0=4, upsampling_steps=3, padding=0.1, mise=True)
    x = torch.from_numpy(synth.tsdf_batch(SCENE, 1))
    c = gen.encode(x)
    lin = torch.from_numpy(gen.mise_lin())
    assert gen.grid_resolution() == 33 == len(lin)
    gx, gy, gz = torch.meshgrid(lin, lin, lin, indexing="ij")
    dense = gen.eval_points(torch.stack((gx, gy, gz), dim=-1).reshape(1, -1, 3).to(DEV), c).reshape(33, 33, 33).cpu().numpy()
    return gen, x, c, dense


def test_no_lattice_value_is_near_the_threshold(e2e):
    gen, _, _, dense = e2e
    margin = np.abs(dense.astype(np.float64) - gen._iso()).min()
    print("nearest lattice value to the threshold:", margin, "= %.1f tau" % (margin / TAU))
    assert margin > 10 * TAU
    assert (dense >= gen._iso()).any() and (dense <= gen._iso()).any()


def test_decoder_in_the_loop_queries_what_the_emulator_derives(e2e):
    gen, _, c, dense = e2e
    want_rounds, want_dense = mise_emu.run(dense, 4, 3, gen._iso())
    assert len(want_rounds) > 2
    seen, rounds, stats = [], [], {}

    def value_fn(q, pts):
        v = gen.eval_points(pts, c)
        seen.append(v)
        return v

    grid = mise_grid(value_fn, 4, 3, gen._iso(), batch=1, device=DEV, lin=torch.from_numpy(gen.mise_lin()).to(DEV), stats=stats,
                     rounds=rounds)
    torch.cuda.synchronize()
    print("round sizes", [cnt[0] for _, cnt in rounds], "emulator", [len(r) for r in want_rounds])
    assert [cnt[0] for _, cnt in rounds] == [len(r) for r in want_rounds]
    worst = 0.0
    for (q, cnt), v, want in zip(rounds, seen, want_rounds):
        idx = q[0, :cnt[0]].cpu().numpy()
        assert np.array_equal(idx, want)
        worst = max(worst, float(np.abs(v[0, :cnt[0]].cpu().numpy().astype(np.float64) - dense.reshape(-1)[idx]).max()))
    print("evaluated samples vs the dense lattice: max abs difference", worst)
    assert worst <= TAU
    assert stats == {"mise rounds": len(want_rounds), "mise points": sum(len(r) for r in want_rounds)}
    assert np.abs(grid[0].cpu().numpy().astype(np.float64) - want_dense).max() <= TAU
    assert torch.equal(grid, gen.value_grid(c))


def test_generate_mesh_with_mise_is_the_mesh_of_the_to_dense_grid(e2e):
    gen, x, c, _ = e2e
    mesh, stats = gen.generate_mesh({"inputs": x})
    assert stats["mise rounds"] > 2 and stats["mise points"] < 33 ** 3 and "time (marching cubes)" in stats
    want = gen.extract_mesh(gen.value_grid(c)[0], c)
    assert len(mesh.vertices) > 0 and mesh.vertices.tobytes() == want.vertices.tobytes() and mesh.faces.tobytes() == want.faces.tobytes()
    batch = gen.generate_meshes(x)
    assert len(batch) == 1 and batch[0].vertices.tobytes() == mesh.vertices.tobytes() and batch[0].faces.tobytes() == mesh.faces.tobytes()
    again = gen.generate_from_latent(c)
    assert again.vertices.tobytes() == mesh.vertices.tobytes()


def test_a_component_inside_one_coarse_cell_is_skipped_by_mise_only(net, e2e):
    _, x, _, dense = e2e
    thr = float(np.log(BALL_THRESHOLD) - np.log(1 - BALL_THRESHOLD))
    assert (dense >= thr).sum() >= 1 and not (dense[::8, ::8, ::8] >= thr).any() and np.abs(dense - thr).min() > 10 * TAU
    kw = dict(device=DEV, threshold=BALL_THRESHOLD, resolution0=4, upsampling_steps=3, padding=0.1)
    sparse, stats = Generator3D(net, mise=True, **kw).generate_mesh({"inputs": x})
    assert stats["mise rounds"] == 1 and stats["mise points"] == 125
    assert sparse.vertices.shape == (0, 3) and sparse.faces.shape == (0, 3) and sparse.vertex_normals is None     # Mesh.empty()
    full = Generator3D(net, mise=False, **kw).generate_mesh({"inputs": x}, return_stats=False)
    assert len(full.vertices) > 0 and len(full.faces) > 0
