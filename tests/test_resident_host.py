"""CPU tests of the resident training set (giga_amd.resident, giga_batch_draw / giga_batch_assemble): the numpy restatement
(tests/resident_emu.py) against the host reader on forced draws, the properties and the uniformity of the occupancy sampler, the
epoch logic of ResidentBatches, and the C ABI's argument checks (made before the first HIP call, so they run without a GPU)."""
import ctypes
import os

import numpy as np
import pytest
import torch
from scipy import ndimage, stats
from scipy.spatial.transform import Rotation

import resident_emu as E
from giga_amd import _capi, resident
from giga_amd.dataset import GraspOccDataset

Z_OFFS = (0.0, 6.0, 6.5, 7.25, 33.99, 39.0, 39.5, 40.0, -3.5)      # exact integers, the floor tie, shifts that empty the grid
BORDER_ROWS = {0: 0, 1: 116, 2: 77, 3: 116}    # output rows (i, j) in range whose source x or y index is exactly 0 or 39


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    paths = E.tiny_sets(str(tmp_path_factory.mktemp("resident")))
    out = {}
    for name, (root, raw) in paths.items():
        ds = GraspOccDataset(root, raw)
        out[name] = (root, raw, resident.host_tables(ds), ds.size)
    return out


class Forced:
    """the reader's generator, returning forced draws in the reader's call order (apply_transform: integers(4), uniform(6, 34);
    _read_occ: integers(n_files), choice(n, size=(M,), replace=M > n)).  `u` is a numpy float64, so that the reader's z_offset is a
    double as in the reference (numpy >= 2 would subtract a float32 from a Python float in float32)."""

    def __init__(self, augment, q, u, k, idx):
        self.todo = ([("integers", 4, q), ("uniform", (6, 34), np.float64(u))] if augment else []) + \
            [("integers", None, k), ("choice", None, np.asarray(idx, np.int64))]

    def _next(self, name):
        assert self.todo and self.todo[0][0] == name, (name, self.todo)
        return self.todo.pop(0)

    def integers(self, high):
        _, want, value = self._next("integers")
        assert want is None or want == high
        assert 0 <= value < high
        return value

    def uniform(self, lo, hi):
        _, want, value = self._next("uniform")
        assert want == (lo, hi)
        return value

    def choice(self, n, size, replace):
        _, _, value = self._next("choice")
        assert value.shape == tuple(size) and value.min() >= 0 and value.max() < n and replace == (size[0] > n)
        return value


def check_grid(got, want, ok, q, what):
    """want: the emulation's grid; got: scipy's.  Bit-equal outside the border set; inside it scipy gives the same value or 0."""
    excluded = E.border_set(q)[:, :, None] & ok
    in_k = int(ok.any(axis=(0, 1)).sum())
    assert int(excluded.sum()) == BORDER_ROWS[q] * in_k, (what, int(excluded.sum()), in_k)
    if ok.any():
        assert excluded.sum() <= 0.10 * ok.sum(), what
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got[~excluded].view(np.uint32), want[~excluded].view(np.uint32)), what
    inside_got, inside_want = got[excluded], want[excluded]
    assert np.all((inside_got == 0) | (inside_got.view(np.uint32) == inside_want.view(np.uint32))), what
    return int(excluded.sum()), int(ok.sum())


@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("M", [1, 7, 2048])
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_emulated_assembly_equals_the_host_reader(sets, name, M, augment):
    root, raw, tables, size = sets[name]
    ds = GraspOccDataset(root, raw, num_point_occ=M, augment=augment)
    assert tables["points"].dtype == (np.float16 if name == "f16" else np.float32)
    rng = np.random.default_rng([11, M, augment])
    n_rows = len(ds)
    quarter = np.arange(n_rows) % 4
    u = rng.uniform(6, 34, n_rows)
    nf = E.files_of(tables, np.arange(n_rows))
    file = (np.arange(n_rows) // 4) % nf                    # every file of every scene that has grasps enough
    excluded = in_range = 0
    sizes_seen = set()
    for i in range(n_rows):
        lo, hi = E.file_range(tables, i, file[i])
        sizes_seen.add(hi - lo)
        idx = E.occ_indices(i, 1, 5, hi - lo, M)
        got = ds.item(i, rng=Forced(augment, int(quarter[i]), u[i], int(file[i]), idx))
        gx, (glabel, grot, gwidth), gpos, gpocc, gocc = got
        want = E.assemble_item(tables["grids"][tables["row_scene"][i]], tables["row_pos"][i], tables["row_quat"][i],
                               tables["row_rotations"][i], tables["row_width"][i], tables["row_label"][i], tables["points"][lo:hi],
                               tables["occ"][lo:hi], size, quarter[i], u[i], idx, augment)
        wx, wpos, wpocc, (wlabel, wrot, wwidth, wocc), ok = want
        what = f"{name} M={M} row {i} q={quarter[i]}"
        assert wlabel == np.float32(glabel) and wwidth == gwidth and np.array_equal(wocc, np.asarray(gocc, np.float32)), what
        assert gpocc.dtype == tables["points"].dtype
        assert np.array_equal(wpocc.view(np.uint32), gpocc.astype(np.float32).view(np.uint32)), what
        if not augment:
            assert ok is None and np.array_equal(wx.view(np.uint32), np.asarray(gx, np.float32).view(np.uint32)), what
            assert np.array_equal(wpos, gpos) and np.array_equal(wrot, grot), what
            continue
        e, r = check_grid(np.asarray(gx, np.float32), wx, ok, int(quarter[i]), what)
        excluded, in_range = excluded + e, in_range + r
        gpos32 = np.asarray(gpos).astype(np.float32)
        assert np.all(np.abs(wpos.astype(np.float64) - gpos32.astype(np.float64)) <= E.ulp32(gpos32)), (what, wpos, gpos)
        assert grot.dtype == np.float32 and np.abs(wrot.astype(np.float64) - grot.astype(np.float64)).max() <= 2.0 ** -24, (what, wrot, grot)
        assert np.all((wrot.astype(np.float64) * grot.astype(np.float64)).sum(axis=1) > 0.0), what
    assert sizes_seen == set(E.FILE_SIZES)
    if augment:
        print(f"{name} M={M}: {excluded} of {in_range} in-range voxels excluded ({100.0 * excluded / in_range:.2f} %)")


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_emulated_grid_equals_scipy_at_forced_shifts(sets, q):
    """z shifts u - z cannot reach, handed to the emulation and to scipy's affine_transform directly (the reader's matrix: the
    inverse of scipy's own rotation; the z offset exactly -z_off)"""
    tables = sets["f32"][2]
    grid = tables["grids"][q % len(tables["grids"])]
    assert len(np.unique(grid)) > 1000
    Ri = Rotation.from_rotvec(np.r_[0.0, 0.0, np.pi / 2.0 * q]).inv().as_matrix()
    centre = np.r_[20.0, 20.0, 20.0]
    for z in Z_OFFS:
        offset = centre - Ri @ centre
        offset[2] = -z
        got = ndimage.affine_transform(grid, Ri, offset, order=0)
        want, ok = E.transform_grid(grid, q, z)
        check_grid(got, want, ok, q, f"q={q} z_off={z}")
        planes = int(ok.any(axis=(0, 1)).sum())
        assert planes == {0.0: 40, 6.0: 34, 6.5: 33, 7.25: 32, 33.99: 6, 39.0: 1, 39.5: 0, 40.0: 0, -3.5: 36}[z], (z, planes)
        if q == 0 and z == 6.5:                               # the tie: c = k - 6.5, floor(c + 0.5) = k - 6
            assert np.array_equal(want[:, :, 7:], grid[:, :, 1:34]) and not want[:, :, :7].any()


# ------------------------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("n", [1, 2, 3, 5, 64, 65, 97, 2047, 2048, 2049, 100000])
def test_sampler_properties(n):
    ordinals = np.arange(6)
    for M in sorted({1, n, min(n, 2048), n + 1}):
        walks = []
        idx = E.occ_indices(ordinals, 2, 9, n, M, walks=walks)
        assert idx.shape == (6, M) and idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < n
        if M <= n:
            assert all(len(np.unique(row)) == M for row in idx)              # distinct; M = n: a permutation of [0, n)
            assert n == 1 or walks[0] <= (1 << E.feistel_bits(n)) - n + 1
        else:
            assert all(len(np.unique(row)) < M for row in idx)               # more draws than values: with replacement
        # a pure function of (seed, epoch, ordinal): one item at a time, in another order, gives the same rows
        for o in (5, 0, 3):
            assert np.array_equal(E.occ_indices(o, 2, 9, n, M), idx[o])
        if n > 1 and M > 1:
            assert not np.array_equal(E.occ_indices(0, 2, 10, n, M), idx[0]) or n <= 3
            assert not np.array_equal(idx[0], idx[1]) or n <= 3


def chi2_bound(cells):
    return stats.chi2.ppf(0.9999, cells - 1)


@pytest.mark.parametrize("n,M,T", [(97, 16, 4000), (5, 3, 4000), (100000, 2048, 50)])
@pytest.mark.parametrize("seed", [0, 1])
def test_sampler_inclusion_counts_are_uniform(n, M, T, seed):
    idx = E.occ_indices(np.arange(T), 0, seed, n, M)
    cnt = np.bincount(idx.reshape(-1), minlength=n).astype(np.float64)
    e = T * M / n
    stat = ((cnt - e) ** 2).sum() / (e * (1.0 - M / n)) * (n - 1) / n
    print(f"n={n} M={M} T={T} seed={seed}: statistic {stat:.1f}, bound {chi2_bound(n):.1f}")
    assert stat < chi2_bound(n)


@pytest.mark.parametrize("seed", [0, 1])
def test_file_and_quarter_draws_are_uniform(seed):
    T = 4000
    for n_files in (2, 3, 7):
        quarter, u, file = E.item_draws(np.arange(T), 0, seed, n_files)
        for what, draws, cells in (("file", file, n_files), ("quarter", quarter, 4)):
            cnt = np.bincount(draws, minlength=cells).astype(np.float64)
            assert len(cnt) == cells
            stat = ((cnt - T / cells) ** 2 / (T / cells)).sum()
            print(f"seed={seed} {what} of {cells}: statistic {stat:.2f}, bound {chi2_bound(cells):.2f}")
            assert stat < chi2_bound(cells)
        assert u.dtype == np.float64 and u.min() >= 6.0 and u.max() < 34.0 and stats.kstest(u, "uniform", args=(6, 28)).pvalue > 1e-4
    # the draws of an item depend on (seed, epoch, ordinal) only
    a = E.item_draws(np.arange(8), 3, seed, 3)
    assert all(np.array_equal(x[5], y[0]) for x, y in zip(a, E.item_draws(np.array([5]), 3, seed, 3)))
    assert not np.array_equal(a[1], E.item_draws(np.arange(8), 4, seed, 3)[1])


# --------------------------------------------------------------------------------------------------------------- epoch logic
@pytest.mark.parametrize("world", [1, 2, 3])
def test_every_row_once_per_epoch_across_ranks(world):
    indices = np.arange(40)
    for epoch in (1, 2):
        parts = [resident.epoch_order(indices, 7, epoch, True, rank, world) for rank in range(world)]
        rows = np.concatenate([p[1] for p in parts])
        ordinals = np.concatenate([p[0] for p in parts])
        assert sorted(rows.tolist()) == list(range(40)) and sorted(ordinals.tolist()) == list(range(40))
        order = np.random.default_rng([7, epoch]).permutation(indices)
        for o, r in zip(ordinals, rows):
            assert order[o] == r                                # an item's ordinal is its place in the epoch's order, on every rank
    with pytest.raises(ValueError):
        resident.epoch_order(indices, 7, 1, True, world, world)


def test_epoch_order_batches_and_subsets():
    sub = np.array([3, 5, 8, 13, 21, 34, 2, 1])
    o1, r1 = resident.epoch_order(sub, 4, 1)
    assert sorted(r1.tolist()) == sorted(sub.tolist()) and np.array_equal(o1, np.arange(8))
    # the order depends on (seed, epoch) only
    assert np.array_equal(r1, resident.epoch_order(sub, 4, 1)[1])
    assert not np.array_equal(r1, resident.epoch_order(sub, 4, 2)[1]) and not np.array_equal(r1, resident.epoch_order(sub, 5, 1)[1])
    assert np.array_equal(resident.epoch_order(sub, 4, 1, shuffle=False)[1], sub)
    assert resident.batch_bounds(40, 32) == [(0, 32), (32, 40)] and resident.batch_bounds(40, 32, drop_last=True) == [(0, 32)]
    assert resident.batch_bounds(64, 32, drop_last=True) == [(0, 32), (32, 64)] and resident.batch_bounds(0, 32) == []
    assert resident.batch_bounds(5, 32) == [(0, 5)] and resident.batch_bounds(5, 32, drop_last=True) == []
    with pytest.raises(ValueError):
        resident.batch_bounds(5, 0)


class FakeSet:
    """what ResidentBatches reads of a set, without a device"""
    augment, num_point_occ, device = True, 8, "cpu"

    def __len__(self):
        return 40


def test_resident_batches_bookkeeping_without_a_device():
    it = resident.ResidentBatches(FakeSet(), 32, seed=3)
    assert len(it) == 2 and it.augment is True and it.epoch == 0
    assert len(resident.ResidentBatches(FakeSet(), 32, drop_last=True, augment=False)) == 1
    assert resident.ResidentBatches(FakeSet(), 32, augment=False).augment is False
    assert [len(resident.ResidentBatches(FakeSet(), 8, rank=r, world=3)) for r in range(3)] == [2, 2, 2]       # 14, 13, 13 rows
    assert len(resident.ResidentBatches(FakeSet(), 8, indices=[1, 2, 3])) == 1
    for bad in (dict(indices=[40]), dict(indices=[-1]), dict(rank=2, world=2), dict(seed=-1), dict(batch_size=0)):
        with pytest.raises(ValueError):
            resident.ResidentBatches(FakeSet(), **{"batch_size": 8, **bad})


# ------------------------------------------------------------------------------------------------------- host side of the set
def test_host_tables_layout_and_guards(sets, tmp_path):
    for name in ("f32", "f16"):
        root, raw, t, size = sets[name]
        ds = GraspOccDataset(root, raw)
        first = list(dict.fromkeys(ds.scene_ids))                # scenes in the order of first appearance in the grasp table
        assert t["grids"].shape == (6, 40, 40, 40) and t["grids"].dtype == np.float32
        assert [first[s] for s in t["row_scene"]] == ds.scene_ids
        assert t["scene_files"].dtype == np.int32 and t["file_points"].dtype == np.int64 and t["occ"].dtype == np.uint8
        f = 0
        for s, sid in enumerate(first):
            assert np.array_equal(t["grids"][s], ds.grid(sid)[0])
            paths = ds.occ_paths(sid)                             # the reader's order, file by file
            assert t["scene_files"][s] == f and t["scene_files"][s + 1] == f + len(paths)
            for p in paths:
                data = np.load(p)
                lo, hi = t["file_points"][f], t["file_points"][f + 1]
                assert np.array_equal(t["points"][lo:hi], data["points"]) and np.array_equal(t["occ"][lo:hi], data["occ"])
                f += 1
        assert f == len(t["file_points"]) - 1 and t["file_points"][-1] == len(t["points"]) == len(t["occ"])
    # a mixed set, a grid of another shape, a scene without files, an empty file: all raise while the set is read
    for case in ("mixed", "shape", "nofiles", "empty"):
        root, raw = str(tmp_path / case / "data"), str(tmp_path / case / "raw")
        E.write_set(root, raw, [[5], [7, 3]], np.float32, grasps_per_scene=2, seed=4, res=20 if case == "shape" else 40)
        d = os.path.join(raw, "occ", "w04_0001")
        if case == "mixed":
            np.savez(os.path.join(d, "0001.npz"), points=np.zeros((3, 3), np.float16), occ=np.zeros(3, bool))
        elif case == "nofiles":
            for f in os.listdir(d):
                os.remove(os.path.join(d, f))
        elif case == "empty":
            np.savez(os.path.join(d, "0001.npz"), points=np.zeros((0, 3), np.float32), occ=np.zeros(0, bool))
        with pytest.raises(ValueError):
            resident.host_tables(GraspOccDataset(root, raw))
        with pytest.raises(ValueError):
            resident.ResidentTrainingSet(GraspOccDataset(root, raw))


def test_no_cpu_fallback(sets):
    root, raw, _, _ = sets["f32"]
    with pytest.raises(_capi.GigaHipError):
        resident.ResidentTrainingSet(GraspOccDataset(root, raw), device="cpu")
    import giga_amd
    assert giga_amd.ResidentTrainingSet is resident.ResidentTrainingSet and giga_amd.ResidentBatches is resident.ResidentBatches


# ------------------------------------------------------------------------------------------------------------------ C ABI
P = 0x10000000                            # never dereferenced: every check precedes the first HIP call


def make_set(**over):
    s = _capi.BatchSet()
    for name, _ in _capi.BatchSet._fields_[:11]:
        setattr(s, name, P)
    s.n_points, s.n_scenes, s.n_rows, s.n_files, s.point_dtype, s.size = 12, 2, 4, 3, 0, 0.3
    keep = []
    for k, v in over.items():
        if isinstance(v, np.ndarray):
            keep.append(v)
            v = v.ctypes.data
        setattr(s, k, v)
    return s, keep


def draw(s, B=2, M=8, epoch=1, ordinals=P, rows=P, outs=(P, P, P, P)):
    return _capi.lib().giga_batch_draw(ctypes.addressof(s) if s is not None else None, ordinals, rows, B, M, epoch, 7, *outs, None)


def assemble(s, B=2, M=8, augment=1, ins=(P, P, P, P, P), outs=(P,) * 7):
    return _capi.lib().giga_batch_assemble(ctypes.addressof(s) if s is not None else None, *ins, B, M, augment, *outs, None)


def test_abi_argument_checks_without_a_gpu():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_batch_draw", "giga_batch_assemble"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (name + "(") in hdr
    assert L.giga_abi_version() == 3
    assert "#define GIGA_BATCH_FEISTEL_ROUNDS %d\n" % E.FEISTEL_ROUNDS in hdr and "#define GIGA_BATCH_RES %d\n" % E.RES in hdr
    assert "#define GIGA_BATCH_MAX_ITEMS %d\n" % _capi.BATCH_MAX_ITEMS in hdr
    for k, v in _capi.BATCH_POINTS.items():
        assert "#define GIGA_BATCH_POINTS_F%s %d\n" % (k[-2:], v) in hdr
    for c in E.SIN_Q + E.COS_Q:
        assert repr(abs(c)) in hdr or c in (0.0, 1.0)
    good, _ = make_set()
    # an empty batch is fine, and checked all the same
    assert draw(good, B=0) == 0 and assemble(good, B=0) == 0
    assert draw(None) == -1 and assemble(None) == -1
    for call in (draw, assemble):
        assert call(good, B=-1) == -1 and call(good, M=-1) == -1 and call(good, B=_capi.BATCH_MAX_ITEMS + 1) == -1
        assert call(good, B=1 << 15, M=1 << 16) == -1                           # B M = 2^31
        for field in ("row_scene", "scene_files", "file_points"):
            assert call(make_set(**{field: None})[0]) == -1
        for field in ("n_points", "n_scenes", "n_rows", "n_files"):
            assert call(make_set(**{field: -1})[0]) == -1
        # host copies of the offsets: they start at 0, do not decrease and end at the counts
        ok_files, ok_points = np.array([0, 1, 3], np.int32), np.array([0, 5, 5, 12], np.int64)
        s, keep = make_set(scene_files_host=ok_files, file_points_host=ok_points)
        assert call(s, B=0) == 0
        for files in ([0, 2, 1], [1, 1, 3], [0, 1, 2], [0, 4, 3]):
            s, keep = make_set(scene_files_host=np.array(files, np.int32))
            assert call(s, B=0) == -1, files
        for points in ([0, 6, 5, 12], [1, 5, 5, 12], [0, 5, 5, 11], [0, -1, 5, 12]):
            s, keep = make_set(file_points_host=np.array(points, np.int64))
            assert call(s, B=0) == -1, points
        s, keep = make_set(file_points_host=np.array([0, 1 << 31, 1 << 31, 1 << 32], np.int64), n_points=1 << 32)
        assert call(s, B=0) == -1                                                # one file holds fewer than 2^31 points
        s, keep = make_set(file_points_host=np.array([0, (1 << 31) - 1, (1 << 32) - 2, (1 << 32) + 5], np.int64), n_points=(1 << 32) + 5)
        assert call(s, B=0) == 0                                                 # ... a set may hold more
    assert draw(good, epoch=-1) == -1 and draw(good, ordinals=None) == -1 and draw(good, rows=None) == -1
    for i in range(4):
        assert draw(good, outs=tuple(None if j == i else P for j in range(4))) == -6
    for field in ("grids", "row_pos", "row_quat", "row_rotations", "row_width", "row_label", "points", "occ"):
        assert assemble(make_set(**{field: None})[0]) == -1 and draw(make_set(**{field: None})[0], B=0) == 0
    assert assemble(make_set(point_dtype=2)[0]) == -1 and assemble(make_set(point_dtype=-1)[0]) == -1
    for bad in (0.0, -0.3, np.nan, np.inf):
        assert assemble(make_set(size=bad)[0]) == -1
    assert assemble(make_set(grids=P + 4)[0]) == -1                              # 16-byte accesses
    for i in (0, 3, 4):                                                          # rows, file, index
        assert assemble(good, ins=tuple(None if j == i else P for j in range(5))) == -1
    for i in (1, 2):                                                             # quarter, u: read only with augmentation
        assert assemble(good, ins=tuple(None if j == i else P for j in range(5))) == -1
    for i in range(7):
        assert assemble(good, outs=tuple(None if j == i else P for j in range(7))) == -6
    assert assemble(good, outs=(P + 8,) + (P,) * 6) == -1
    assert L.giga_strerror(-6) == b"null pointer for a requested output"
