"""GPU tests of the mesh simplification (csrc/giga_simplify.hip through giga_mesh_simplify / giga_amd.mesh.simplify_mesh) on the
fixtures of tests/golden/g20_simplify.npz: the output of the reference's Simplify.h driven stand-alone on value-initialised records
(tools/make_simplify_goldens.py), byte for byte; the overflow path of the reference lists, batches, the face-index check and
`Generator3D(simplify_nfaces=N)` end to end.  Reads only tests/golden/."""
import numpy as np
import pytest
import torch

from giga_amd import _capi, networks, synth, weights
from giga_amd.generation import Generator3D
from giga_amd.mesh import simplify_mesh

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ["tetra_2", "octa_4", "ico2_160", "ico2_32", "ico2_6", "torus_576", "torus_114", "torus_7", "cap_404", "cap_80", "cap_7",
         "mc17_f2", "mc17_f10", "mc33_f2", "mc33_f10", "unref_40", "ico2_keep", "unref_keep", "ico1_0"]


@pytest.fixture(scope="module")
def g20(golden):
    return golden("g20_simplify.npz")


@pytest.fixture(scope="module")
def net():
    n = networks.get_network("giga")
    n.load_state_dict(weights.make_state_dict(7))
    return n.to(DEV).eval()


def _inputs(g20, name):
    return (torch.from_numpy(g20[name + "_vertices_in"]).to(DEV), torch.from_numpy(g20[name + "_faces_in"]).to(DEV),
            int(g20[name + "_target"]), float(g20[name + "_agressiveness"]))


def _run(g20, name, **kw):
    v, f, target, aggr = _inputs(g20, name)
    ov, of, counts = simplify_mesh(v, f, target, aggr, **kw)
    assert ov.is_cuda and of.is_cuda and counts.is_cuda and ov.dtype == torch.float64 and of.dtype == torch.int32
    assert counts.tolist() == [[ov.shape[0], of.shape[0]]]
    return ov.cpu().numpy(), of.cpu().numpy()


def _assert_golden(g20, name, ov, of):
    assert ov.shape == g20[name + "_vertices"].shape and of.shape == g20[name + "_faces"].shape, name
    assert of.tobytes() == g20[name + "_faces"].tobytes(), name
    assert ov.tobytes() == g20[name + "_vertices"].tobytes(), name


@pytest.mark.parametrize("name", NAMES)
def test_kernels_match_the_reference_byte_for_byte(g20, name):
    stats = {}
    ov, of = _run(g20, name, stats=stats)
    print(name, "stats", stats)
    _assert_golden(g20, name, ov, of)
    # the schedule is the emulator's: iterations, rounds and repeated passes as tools/make_simplify_goldens.py recorded them
    assert [stats["iterations"][0], stats["rounds"][0], stats["repeated passes"][0]] == g20[name + "_stats"][:3].tolist()
    assert stats["list rebuilds"] == [0]


def test_more_than_1024_vertices_against_the_emulator(golden):
    """No mesh of g20 has more than 1024 vertices (its largest, mc33, has 700; torus and mc33 have more than 1024 faces).  Mesh A of
    g16_mesh.npz, the smallest of tests/golden/ that has them (2084 vertices, 4168 faces), takes the per-mesh scans over the
    vertices into a third round of 1024; the float64 emulator of tests/simplify_emu.py is the reference."""
    import mesh_emu
    import simplify_emu
    g16 = golden("g16_mesh.npz")
    v, f = mesh_emu.marching_cubes(g16["A_grid"], float(g16["A_iso"]), float(g16["A_box_size"]))
    assert (len(v), len(f)) == (2084, 4168) and np.array_equal(mesh_emu.sort_rows(v), g16["A_vertices"])
    ev, ef = simplify_emu.simplify(v, f, 2000, 5.0)
    assert len(ef) == 2000 and len(ev) > 900
    ov, of, counts = simplify_mesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), 2000, 5.0)
    assert counts.tolist() == [[len(ev), len(ef)]]
    assert of.cpu().numpy().tobytes() == np.asarray(ef, np.int32).tobytes()
    assert ov.cpu().numpy().tobytes() == np.asarray(ev, np.float64).tobytes()


def test_float64_input_gives_the_same_bytes(g20):
    v, f, target, aggr = _inputs(g20, "ico2_32")
    ov, of, _ = simplify_mesh(v.double(), f.long(), target, aggr)
    assert of.dtype == torch.int64
    _assert_golden(g20, "ico2_32", ov.cpu().numpy(), of.cpu().numpy().astype(np.int32))


def test_smallest_reference_list_capacity_rebuilds_and_gives_the_same_bytes(g20):
    for name in ("ico2_160", "ico2_32", "ico2_6"):
        stats = {}
        ov, of = _run(g20, name, stats=stats, ref_extra=_capi.SIMPLIFY_MIN_REF_EXTRA)
        print(name, "stats", stats)
        _assert_golden(g20, name, ov, of)
        assert stats["list rebuilds"][0] >= 1
    with pytest.raises(_capi.GigaHipError):
        _run(g20, "ico2_32", ref_extra=_capi.SIMPLIFY_MIN_REF_EXTRA - 1)


def _batch(g20, names):
    vs, fs, counts, targets = [], [], [], []
    for n in names:
        if n is None:                                                   # an empty mesh
            counts.append((0, 0))
            targets.append(10)
            continue
        v, f, t, aggr = _inputs(g20, n)
        assert aggr == 5.0
        vs.append(v)
        fs.append(f)
        counts.append((len(v), len(f)))
        targets.append(t)
    stats = {}
    ov, of, oc = simplify_mesh(torch.cat(vs), torch.cat(fs), targets, 5.0, counts=torch.tensor(counts), stats=stats)
    oc = oc.cpu()
    assert tuple(oc.shape) == (len(names), 2) and int(oc[:, 0].sum()) == len(ov) and int(oc[:, 1].sum()) == len(of)
    ve, fe = oc[:, 0].cumsum(0).tolist(), oc[:, 1].cumsum(0).tolist()
    ov, of = ov.cpu().numpy(), of.cpu().numpy()
    return [(ov[ve[b] - int(oc[b, 0]):ve[b]], of[fe[b] - int(oc[b, 1]):fe[b]]) for b in range(len(names))], stats


@pytest.mark.parametrize("names", [("tetra_2", "torus_114", "mc17_f10"), ("tetra_2", None, "torus_114", "mc17_f10")])
def test_batch_of_three_meshes_equals_the_single_runs(g20, names):
    out, stats = _batch(g20, names)
    for n, (ov, of), it, rounds in zip(names, out, stats["iterations"], stats["rounds"]):
        if n is None:
            assert ov.shape == (0, 3) and of.shape == (0, 3) and it == 0 and rounds == 0
            continue
        _assert_golden(g20, n, ov, of)                                  # (the single run gives the golden: first test)
        assert [it, rounds] == g20[n + "_stats"][:2].tolist()


def test_four_copies_take_the_rounds_of_one(g20):
    out, stats = _batch(g20, ["torus_114"] * 4)
    for ov, of in out:
        _assert_golden(g20, "torus_114", ov, of)
    one = g20["torus_114_stats"]
    assert stats["iterations"] == [int(one[0])] * 4 and stats["rounds"] == [int(one[1])] * 4
    assert stats["repeated passes"] == [int(one[2])] * 4


def test_face_index_out_of_range_raises_and_the_next_call_is_sound(g20):
    v, f, target, aggr = _inputs(g20, "ico2_32")
    for bad in (len(v), -1, 2 ** 30):
        g = f.clone()
        g[17, 1] = bad
        with pytest.raises(_capi.GigaHipError, match="vertex range"):
            simplify_mesh(v, g, target, aggr)
    # in a batch an index is held against its OWN mesh's range
    with pytest.raises(_capi.GigaHipError, match="vertex range"):
        g = f.clone()
        g[0, 0] = len(v) - 1
        simplify_mesh(torch.cat((v[:-1], v)), torch.cat((g, f)), target, aggr, counts=[(len(v) - 1, len(f)), (len(v), len(f))])
    ov, of = _run(g20, "ico2_32")
    _assert_golden(g20, "ico2_32", ov, of)


def test_empty_mesh_and_target_above_the_face_count():
    ov, of, counts = simplify_mesh(torch.zeros((0, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV), 10)
    assert tuple(ov.shape) == (0, 3) and tuple(of.shape) == (0, 3) and counts.tolist() == [[0, 0]]
    ov, of, counts = simplify_mesh(torch.rand((5, 3), device=DEV), torch.zeros((0, 3), dtype=torch.int32, device=DEV), 10)
    assert tuple(ov.shape) == (0, 3) and counts.tolist() == [[0, 0]]   # vertices no face refers to are dropped


N_FACES = 4000           # (the synthetic weights' 33^3 mesh has several times as many faces and can be brought below this)


def _generators(net):
    kw = dict(device=DEV, threshold=0.6, resolution0=4, upsampling_steps=3, with_normals=True)      # a 33^3 value grid
    return Generator3D(net, simplify_nfaces=N_FACES, **kw), Generator3D(net, **kw)


def test_generator_simplifies_after_the_normals(net):
    net.set_precision("fp32")
    gen, plain = _generators(net)
    assert gen.grid_resolution() == 33
    data = {"inputs": torch.from_numpy(synth.tsdf_batch(40, 1))}
    mesh, stats = gen.generate_mesh(data)
    full = plain.generate_mesh(data, return_stats=False)
    assert len(full.faces) > N_FACES and full.vertex_normals is not None
    ev, ef, _ = simplify_mesh(torch.from_numpy(full.vertices).to(DEV), torch.from_numpy(full.faces).to(DEV), N_FACES, 5.)
    assert 0 < len(mesh.faces) <= N_FACES and mesh.vertex_normals is None
    assert mesh.vertices.dtype == np.float32 and mesh.faces.dtype == np.int64
    assert mesh.faces.tobytes() == ef.cpu().numpy().tobytes()
    assert mesh.vertices.tobytes() == ev.float().cpu().numpy().tobytes()
    assert "time (simplify)" in stats and "time (normals)" in stats and "time (simplify)" not in plain.generate_mesh(data)[1]


def test_generate_meshes_with_simplification_equals_single_calls(net):
    net.set_precision("fp16x3")
    try:
        gen, _ = _generators(net)
        x = torch.from_numpy(synth.tsdf_batch(40, 2))
        batch = gen.generate_meshes(x)
        assert len(batch) == 2
        for b in range(2):
            one = gen.generate_mesh({"inputs": x[b:b + 1]}, return_stats=False)
            assert 0 < len(one.faces) <= N_FACES and one.vertex_normals is None and batch[b].vertex_normals is None
            assert one.vertices.tobytes() == batch[b].vertices.tobytes(), b
            assert one.faces.tobytes() == batch[b].faces.tobytes(), b
    finally:
        net.set_precision("fp32")
