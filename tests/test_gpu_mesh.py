"""GPU tests of the mesh extraction: giga_mesh_count / giga_mesh_emit (csrc/giga_mesh.hip) on the fixtures of
tests/golden/g16_mesh.npz (the reference's libmcubes, tools/make_mesh_goldens.py) and against the numpy restatement of
tests/mesh_emu.py; Generator3D.generate_mesh / generate_meshes end to end.  Reads only tests/golden/."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import networks, synth, weights
from giga_amd.generation import Generator3D
from giga_amd.mesh import marching_cubes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_emu  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["A", "B", "C0", "C1", "C2", "C3"]


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_mesh.npz")


@pytest.fixture(scope="module")
def net():
    n = networks.get_network("giga")
    n.load_state_dict(weights.make_state_dict(7))
    return n.to(DEV).eval()


def _run(grid, iso, box):
    v, t, counts = marching_cubes(torch.from_numpy(np.ascontiguousarray(grid)).to(DEV)[None], iso, box)
    torch.cuda.synchronize()
    assert counts.shape == (1, 2) and tuple(v.shape) == (int(counts[0, 0]), 3) and tuple(t.shape) == (int(counts[0, 1]), 3)
    return v.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", NAMES)
def test_kernels_match_the_reference_and_the_emulation(g16, name):
    grid, iso, box = g16[name + "_grid"], float(g16[name + "_iso"]), float(g16[name + "_box_size"])
    v, f = _run(grid, iso, box)
    nv, nf = (int(x) for x in g16[name + "_counts"])
    assert v.dtype == np.float32 and f.dtype == np.int32 and len(v) == nv
    if nv:
        err = np.abs(mesh_emu.sort_rows(v).astype(np.float64) - g16[name + "_vertices"].astype(np.float64)).max()
        print(name, "max vertex error vs reference", err)
        assert err <= 2e-6
    if int(g16[name + "_ambiguous_faces"]) == 0:
        assert len(f) == nf
        assert mesh_emu.euler_characteristic(nv, f) == int(g16[name + "_euler"])
    assert mesh_emu.closed_and_oriented(nv, f)
    assert np.sign(mesh_emu.signed_volume(v, f)) == int(g16[name + "_volume_sign"])
    ev, ef = mesh_emu.marching_cubes(grid, iso, box)
    assert np.array_equal(f, ef)                                   # same cells, same order, same indices
    assert ev.dtype == v.dtype and v.tobytes() == ev.tobytes()     # ... and the same vertex bits
    v2, f2 = _run(grid, iso, box)                                  # a second run: the same bytes
    assert v.tobytes() == v2.tobytes() and f.tobytes() == f2.tobytes()


def test_batch_equals_one_at_a_time(g16):
    """Grids stacked as one batch (the four 5x6x7 grids; A and B, both 32^3) give, scene by scene, the bytes of single calls."""
    for names, iso, box in ((["C0", "C1", "C2", "C3", "C1"], float(g16["C1_iso"]), 1.1), (["A", "B", "A"], float(g16["B_iso"]), 1.0)):
        grids = torch.from_numpy(np.stack([g16[n + "_grid"] for n in names])).to(DEV)
        v, t, counts = marching_cubes(grids, iso, box)
        torch.cuda.synchronize()
        v, t = v.cpu().numpy(), t.cpu().numpy()
        v0 = t0 = 0
        for b, n in enumerate(names):
            sv, st = _run(g16[n + "_grid"], iso, box)
            nv, nt = int(counts[b, 0]), int(counts[b, 1])
            assert (nv, nt) == (len(sv), len(st)), n
            assert v[v0:v0 + nv].tobytes() == sv.tobytes() and t[t0:t0 + nt].tobytes() == st.tobytes(), n
            v0, t0 = v0 + nv, t0 + nt
        assert (v0, t0) == (len(v), len(t))


def test_capacity_one_short_is_reported_and_guards_stay(g16):
    from giga_amd import _capi
    grids = torch.from_numpy(np.stack([g16["A_grid"], g16["B_grid"]])).to(DEV)
    iso = float(g16["B_iso"])
    full_v, full_t, counts = marching_cubes(grids, iso, 1.0)
    nv, nt = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    L = _capi.lib()
    ws = torch.empty(L.giga_mesh_workspace_bytes(2, 32, 32, 32), dtype=torch.uint8, device=DEV)
    cnt = torch.zeros((2, 2), dtype=torch.int32, device=DEV)
    GUARD = 64
    for short_v, short_t in ((1, 0), (0, 1), (1, 1), (0, 0)):
        vbuf = torch.full(((nv - short_v) * 3 + GUARD,), -777.0, device=DEV)
        tbuf = torch.full(((nt - short_t) * 3 + GUARD,), -777, dtype=torch.int32, device=DEV)
        sf = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        _capi.check(L.giga_mesh_count(_capi.ptr(grids), 2, 32, 32, 32, iso, _capi.ptr(ws), ws.numel(), _capi.ptr(cnt),
                                      _capi.stream_ptr(DEV)), "count")
        _capi.check(L.giga_mesh_emit(_capi.ptr(grids), 2, 32, 32, 32, iso, 1.0, _capi.ptr(ws), ws.numel(), _capi.ptr(vbuf),
                                     nv - short_v, _capi.ptr(tbuf), nt - short_t, _capi.ptr(sf), _capi.stream_ptr(DEV)), "emit")
        torch.cuda.synchronize()
        assert sf.tolist() == [short_v, short_t]
        assert torch.equal(cnt.cpu().to(torch.int64), counts)
        assert bool((vbuf[(nv - short_v) * 3:] == -777.0).all()) and bool((tbuf[(nt - short_t) * 3:] == -777).all())
        assert torch.equal(vbuf[:(nv - short_v) * 3].view(-1, 3), full_v[:nv - short_v])
        assert torch.equal(tbuf[:(nt - short_t) * 3].view(-1, 3), full_t[:nt - short_t])


def test_non_cubic_and_cpu_inputs():
    from giga_amd._capi import GigaHipError
    with pytest.raises(GigaHipError):
        marching_cubes(torch.zeros(1, 8, 8, 8), 0.0)
    rng = np.random.default_rng(5)
    grid = rng.standard_normal((9, 17, 66)).astype(np.float32)      # 66 + 1 cells: a row is longer than a wave
    v, f = _run(grid, 0.1, 1.3)
    ev, ef = mesh_emu.marching_cubes(grid, 0.1, 1.3)
    assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes()
    assert mesh_emu.closed_and_oriented(len(v), f) and len(v) == len(mesh_emu.crossed_edges(grid, 0.1))


def _ball_at_the_far_face(shape, radius=9.0):
    """radius - distance, in samples, from the middle of the x = nx - 1 face: a half ball that the padding closes with a cap.
    Its crossed edges lie in the last x-slabs of cells, the cap's in the very last one, so the workgroups with the highest numbers
    have counts, and every workgroup before them holds a share of the ball."""
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    c = (shape[0] - 1, (shape[1] - 1) / 2 + 0.25, (shape[2] - 1) / 2 - 0.25)
    return (radius - np.sqrt((i - c[0]) ** 2 + (j - c[1]) ** 2 + (k - c[2]) ** 2)).astype(np.float32)


@pytest.mark.parametrize("shape, nblk", [((63, 63, 63), 1024), ((63, 63, 64), 1040)], ids=["one-full-round", "second-round"])
def test_scene_offsets_over_a_thousand_workgroup_sums(shape, nblk):
    """The scan of a scene's workgroup sums runs in rounds of 1024: exactly one full round, and 16 sums into a second one."""
    cells = (shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1)
    assert -(-cells // 256) == nblk
    grid = _ball_at_the_far_face(shape)
    ev, ef = mesh_emu.marching_cubes(grid, 0.125, 1.0)
    last = mesh_emu.edges_in_kernel_order(grid, 0.125)[-1]
    assert last[:2] == (0, shape[0]) and 500 < len(ev) < 5000        # the last vertex: an x edge into the padding, last slab of cells
    v, f = _run(grid, 0.125, 1.0)
    assert np.array_equal(f, ef) and v.tobytes() == ev.tobytes()
    assert mesh_emu.closed_and_oriented(len(v), f)


def test_bases_over_more_than_a_wave_of_scenes():
    """65 scenes of 3x3x3 samples, every fourth one empty: the bases of the scenes are taken 64 at a time, scene 64 in a second
    round."""
    rng = np.random.default_rng(65)
    grids = rng.standard_normal((65, 3, 3, 3)).astype(np.float32)
    grids[1::4] = -5.0
    v, t, counts = marching_cubes(torch.from_numpy(grids).to(DEV), 0.1, 1.2)
    torch.cuda.synchronize()
    v, t, counts = v.cpu().numpy(), t.cpu().numpy(), counts.cpu().numpy()
    assert counts.shape == (65, 2) and (counts[1::4] == 0).all() and (counts[63:] > 0).all()      # scene 64 is not empty
    v0 = t0 = 0
    for b in range(65):
        ev, ef = mesh_emu.marching_cubes(grids[b], 0.1, 1.2)
        nv, nt = int(counts[b, 0]), int(counts[b, 1])
        assert (nv, nt) == (len(ev), len(ef)), b
        assert v[v0:v0 + nv].tobytes() == ev.tobytes() and t[t0:t0 + nt].tobytes() == ef.tobytes(), b
        v0, t0 = v0 + nv, t0 + nt
    assert (v0, t0) == (len(v), len(t))


def _along_axis(vertices, edges, n, box):
    """{edge: position of its vertex along the edge's axis, in grid steps}; `edges` names the vertices' edges in order."""
    assert len(vertices) == len(edges)
    g = (vertices.astype(np.float64) / box + 0.5) * (n - 1)
    return {e: g[r, e[0]] for r, e in enumerate(edges)}


def _compare_with_grid_tolerance(grid, mesh, ref_grid, ref_vertices, ref_edge_order, iso, n, box, label):
    """The issue's end-to-end criterion for a mesh made from `grid` against one made from `ref_grid` (grids within 1e-4):
    the crossed edges are the same except edges with an end within 1e-4 of the threshold in the reference grid; the
    vertices of every other common edge differ by at most 2e-4 / |f2 - f1| grid steps.  The output order is cell order,
    then the x / y / z edge, so `edges_in_kernel_order` names the edge of every vertex."""
    assert np.abs(grid.astype(np.float64) - ref_grid).max() <= 1e-4
    ref_edges, near = set(ref_edge_order), mesh_emu.near_threshold_edges(ref_grid, iso)
    got_order = mesh_emu.edges_in_kernel_order(grid, iso)
    got_edges = set(got_order)
    assert got_edges == mesh_emu.crossed_edges(grid, iso) and len(got_order) == len(got_edges)
    pad = np.pad(ref_grid, 1, constant_values=mesh_emu.PAD).astype(np.float64)

    def ends(e):
        q = list(e[1:])
        q[e[0]] += 1
        return pad[e[1], e[2], e[3]], pad[q[0], q[1], q[2]]

    diff = ref_edges ^ got_edges
    print(label, "crossed edges: reference", len(ref_edges), "this", len(got_edges), "differ", len(diff), "near-threshold", len(near))
    assert all(min(abs(f - iso) for f in ends(e)) <= 1e-4 for e in diff)
    got = _along_axis(mesh.vertices, got_order, n, box)
    ref = _along_axis(ref_vertices, ref_edge_order, n, box)
    worst, compared = 0.0, 0
    for e, p in ref.items():
        if e in near or e not in got:
            continue
        f1, f2 = ends(e)
        bound = 2e-4 / abs(f2 - f1)
        worst, compared = max(worst, abs(got[e] - p) / bound), compared + 1
        assert abs(got[e] - p) <= bound, (e, got[e], p, f1, f2)
    print(label, "vertices compared:", compared, "of", len(ref_edges), "worst |d| / bound", worst)
    assert compared >= len(ref_edges) - len(near) - len(diff)


def test_generate_mesh_end_to_end(g16, net):
    """generate_mesh from the TSDF of scene 70 at fixture B's settings (resolution0 32, no upsampling, padding 0, its threshold)."""
    net.set_precision("fp32")
    th, iso = float(g16["B_threshold"]), float(g16["B_iso"])
    gen = Generator3D(net, device=DEV, threshold=th, resolution0=32, upsampling_steps=0, padding=0.0)
    x = torch.from_numpy(synth.tsdf_batch(70, 1))
    c = gen.encode(x)
    grid = gen.value_grid(c)[0].cpu().numpy()
    ref_grid = g16["B_grid"]
    gerr = np.abs(grid.astype(np.float64) - ref_grid).max()
    print("device grid vs fixture: max abs error", gerr)
    assert gerr <= 1e-4
    mesh, stats = gen.generate_mesh({"inputs": x})
    assert mesh.vertices.dtype == np.float32 and mesh.faces.dtype == np.int64 and mesh.vertex_normals is None
    assert {"time (encode inputs)", "time (eval points)", "time (marching cubes)"} <= set(stats)
    assert mesh_emu.closed_and_oriented(len(mesh.vertices), mesh.faces)
    assert np.sign(mesh_emu.signed_volume(mesh.vertices, mesh.faces)) == int(g16["B_volume_sign"])
    # the reference's vertices keyed by edge: the emulation on the fixture's grid gives the fixture's vertices bit for bit, and
    # gives them in edge order
    ref_v, _ = mesh_emu.marching_cubes(ref_grid, iso, 1.0)
    assert np.array_equal(mesh_emu.sort_rows(ref_v), g16["B_vertices"])
    ref_order = mesh_emu.edges_in_kernel_order(ref_grid, iso)
    assert len(mesh_emu.near_threshold_edges(ref_grid, iso)) <= 0.01 * len(ref_order)
    _compare_with_grid_tolerance(grid, mesh, ref_grid, ref_v, ref_order, iso, 32, 1.0, "scene 70 vs reference:")
    # normals
    gen_n = Generator3D(net, device=DEV, threshold=th, resolution0=32, upsampling_steps=0, padding=0.0, with_normals=True)
    mesh_n = gen_n.generate_mesh({"inputs": x}, return_stats=False)
    assert mesh_n.vertices.tobytes() == mesh.vertices.tobytes() and mesh_n.faces.tobytes() == mesh.faces.tobytes()
    assert mesh_n.vertex_normals.shape == mesh.vertices.shape and mesh_n.vertex_normals.dtype == np.float32
    assert np.abs(np.linalg.norm(mesh_n.vertex_normals.astype(np.float64), axis=1) - 1).max() < 1e-5
    assert np.array_equal(mesh_n.vertex_normals, gen.estimate_normals(torch.from_numpy(mesh.vertices).to(DEV), c))
    # extract_mesh on the device grid is the same mesh; a grid below the threshold everywhere is the empty mesh
    again = gen.extract_mesh(gen.value_grid(c)[0], c)
    assert again.vertices.tobytes() == mesh.vertices.tobytes() and again.faces.tobytes() == mesh.faces.tobytes()
    empty = gen.extract_mesh(torch.full((8, 8, 8), -50.0, device=DEV))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)


def test_generate_meshes_equals_single_calls(net):
    """Four scenes in one call against four single calls, byte for byte.  The f16x3 mode is the fp32-grade precision whose
    encoder the library states to be independent of the batch size (the fp32 encoder's conv_in summation order follows the
    batch: INTEGRATION.md section 4)."""
    net.set_precision("fp16x3")
    try:
        gen = Generator3D(net, device=DEV, threshold=0.6, resolution0=32, upsampling_steps=0, with_normals=True)
        x = torch.from_numpy(synth.tsdf_batch(40, 4))
        batch = gen.generate_meshes(x)
        assert len(batch) == 4
        for b in range(4):
            one = gen.generate_mesh({"inputs": x[b:b + 1]}, return_stats=False)
            assert len(one.vertices) > 0
            assert one.vertices.tobytes() == batch[b].vertices.tobytes(), b
            assert one.faces.tobytes() == batch[b].faces.tobytes(), b
            assert one.vertex_normals.tobytes() == batch[b].vertex_normals.tobytes(), b
    finally:
        net.set_precision("fp32")


def test_generate_meshes_fp32_against_single_calls(net):
    """fp32, the default precision: the encoder's summation order follows the batch size, so the planes of scene b in a batch
    and alone agree at rounding level only.  Four scenes in one call against four single calls with the end-to-end
    criterion: value grids within 1e-4 (printed: far inside), the same crossed edges away from the threshold, vertices
    within 2e-4 / |f2 - f1| grid steps, every mesh closed and oriented."""
    net.set_precision("fp32")
    gen = Generator3D(net, device=DEV, threshold=0.6, resolution0=32, upsampling_steps=0)
    x = torch.from_numpy(synth.tsdf_batch(40, 4))
    iso, box = gen._iso(), 1 + gen.padding
    c = gen.encode(x)
    grids = gen.value_grid(c).cpu().numpy()
    batch = gen.generate_meshes(x)
    assert len(batch) == 4
    for b in range(4):
        cb = gen.encode(x[b:b + 1])
        gb = gen.value_grid(cb)[0].cpu().numpy()
        one = gen.generate_mesh({"inputs": x[b:b + 1]}, return_stats=False)
        print("scene", b, "grid in the batch vs alone: max abs difference", np.abs(grids[b].astype(np.float64) - gb).max())
        assert len(batch[b].vertices) > 0 and mesh_emu.closed_and_oriented(len(batch[b].vertices), batch[b].faces)
        assert mesh_emu.closed_and_oriented(len(one.vertices), one.faces)
        _compare_with_grid_tolerance(grids[b], batch[b], gb, one.vertices, mesh_emu.edges_in_kernel_order(gb, iso), iso, 32, box,
                                     "scene %d batch vs alone:" % b)


def test_generate_meshes_above_the_lattice_limit(net):
    """Two scenes at 73 samples per axis (resolution0 9, three upsampling steps): the generic decoder on the shared points
    expanded over the batch.  Against single calls with the same criterion as above."""
    net.set_precision("fp32")
    gen = Generator3D(net, device=DEV, threshold=0.6, resolution0=9, upsampling_steps=3, with_normals=True)
    n = gen.grid_resolution()
    assert n == 73
    x = torch.from_numpy(synth.tsdf_batch(40, 2))
    iso, box = gen._iso(), 1 + gen.padding
    grids = gen.value_grid(gen.encode(x))
    assert tuple(grids.shape) == (2, n, n, n)
    grids = grids.cpu().numpy()
    batch = gen.generate_meshes(x)
    for b in range(2):
        gb = gen.value_grid(gen.encode(x[b:b + 1]))[0].cpu().numpy()
        one = gen.generate_mesh({"inputs": x[b:b + 1]}, return_stats=False)
        m = batch[b]
        assert len(m.vertices) > 0 and mesh_emu.closed_and_oriented(len(m.vertices), m.faces)
        assert m.vertex_normals.shape == m.vertices.shape
        assert np.abs(np.linalg.norm(m.vertex_normals.astype(np.float64), axis=1) - 1).max() < 1e-5
        _compare_with_grid_tolerance(grids[b], m, gb, one.vertices, mesh_emu.edges_in_kernel_order(gb, iso), iso, n, box,
                                     "73^3 scene %d batch vs alone:" % b)


def test_default_setting_runs_and_is_closed(net):
    """The reference's defaults: resolution0 16, three upsampling steps -> 129^3 samples, padding 0.1."""
    net.set_precision("fp32")
    gen = Generator3D(net, device=DEV, threshold=0.6)
    assert gen.grid_resolution() == 129
    mesh, stats = gen.generate_mesh({"inputs": torch.from_numpy(synth.tsdf_batch(70, 1))})
    print("129^3:", len(mesh.vertices), "vertices", len(mesh.faces), "faces", stats)
    assert len(mesh.vertices) > 0
    assert np.abs(mesh.vertices).max() <= 0.55 * (1 + 2.0 / 128) + 1e-6
    assert mesh_emu.closed_and_oriented(len(mesh.vertices), mesh.faces)
