"""GPU tests of the resident training set (csrc/giga_batch.hip through giga_amd.resident) against the numpy restatement
(tests/resident_emu.py, itself held to the host reader by tests/test_resident_host.py): the draws and the assembly bit for bit,
batch independence, untouched inputs, the iterator, the guards, and one training step on a yielded batch."""
import numpy as np
import pytest
import torch

import resident_emu as E
from giga_amd import _capi, dataset, networks, resident
from giga_amd.dataset import GraspOccDataset
from giga_amd.training import giga_loss

pytestmark = pytest.mark.gpu

Z_OFFS = (0.0, 6.0, 6.5, 7.25, 33.99, 39.0, 39.5, 40.0, -3.5)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    """name -> (dataset, resident set, host tables): the tiny sets of the host tests, uploaded once"""
    dev = torch.device("cuda:0")
    out = {}
    for name, (root, raw) in E.tiny_sets(str(tmp_path_factory.mktemp("resident"))).items():
        ds = GraspOccDataset(root, raw, num_point_occ=64, augment=True)
        out[name] = (ds, resident.ResidentTrainingSet(ds, device=dev), resident.host_tables(ds))
    return out


def dev_ints(a, dev):
    return torch.from_numpy(np.asarray(a, np.int32)).to(dev)


def bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a


def flat(batch):
    x, pos, pos_occ, (label, rot, width, occ) = batch
    return dict(x=x, pos=pos, pos_occ=pos_occ, label=label, rot=rot, width=width, occ=occ)


@pytest.mark.parametrize("name", ["sizes", "f16"])
@pytest.mark.parametrize("M", [1, 7, 2048])
def test_draws_equal_the_emulation(sets, name, M):
    """every file size of SAMPLER_SIZES ("sizes": one file per scene) and scenes with several files ("f16"), at B = 1, 3, 32, 33,
    two seeds, epochs 0 and 3; rows and ordinals in an order of their own"""
    ds, rset, tables = sets[name]
    rng = np.random.default_rng([21, M])
    seen = set()
    for B in (1, 3, 32, 33):
        for seed, epoch in ((0, 0), ((1 << 63) + 12345, 3)):
            rows = rng.integers(0, len(ds), B) if B < 32 else rng.permutation(len(ds))[:B]
            ordinals = rng.permutation(1000)[:B]
            want = E.draw_batch(tables, ordinals, epoch, seed, rows, M)
            got = rset.draw(dev_ints(ordinals, rset.device), epoch, seed, dev_ints(rows, rset.device), M)
            assert [g.dtype for g in got] == [torch.int32, torch.float64, torch.int32, torch.int32]
            assert [tuple(g.shape) for g in got] == [(B,), (B,), (B,), (B, M)]
            for what, g, w in zip(("quarter", "u", "file", "index"), got, want):
                assert np.array_equal(bits(g), bits(w)), (what, B, seed, epoch)
            for b in range(B):
                lo, hi = E.file_range(tables, rows[b], want[2][b])
                seen.add(hi - lo)
    assert seen == set(E.SAMPLER_SIZES if name == "sizes" else E.FILE_SIZES)


def forced_draws(tables, rows, M, rng, z_offs=None):
    """quarter turns in turn, every file, indices from the emulated sampler; u uniform, or z_off + z for the listed shifts"""
    B = len(rows)
    quarter = (np.arange(B) % 4).astype(np.int32)
    file = ((np.arange(B) // 4) % E.files_of(tables, rows)).astype(np.int32)
    u = rng.uniform(6, 34, B)
    if z_offs is not None:
        u = np.asarray(z_offs, np.float64) + tables["row_pos"][rows, 2].astype(np.float64)
    index = np.stack([E.occ_indices(b, 1, 3, np.diff(E.file_range(tables, rows[b], file[b]))[0], M) for b in range(B)])
    return quarter, u, file, index.astype(np.int32)


def check_batch(got, want, augment, what):
    got, want = flat(got), flat(want)
    for k in ("x", "pos_occ", "label", "width", "occ") + (() if augment else ("pos", "rot")):
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == want[k].shape, (what, k)
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)
    if augment:
        # the double-precision chains of pos and rot: one IEEE rounding per operation on both sides (the kernels are compiled
        # without contraction); a fused multiply-add would move the final float32 rounding by at most one ulp
        for k in ("pos", "rot"):
            g, w = got[k].cpu().numpy(), want[k]
            assert g.shape == w.shape and g.dtype == np.float32
            err = np.abs(g.astype(np.float64) - w.astype(np.float64)) / E.ulp32(w)
            print(f"{what} {k}: max {err.max():.3g} ulp, {int((err > 0).sum())} of {err.size} differ")
            assert err.max() <= 1.0, (what, k)


@pytest.mark.parametrize("name", ["f32", "f16"])
@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_assembly_equals_the_emulation(sets, name, augment):
    ds, rset, tables = sets[name]
    dev = rset.device
    rng = np.random.default_rng([22, augment])
    for M in (1, 7, 2048):
        rows = rng.permutation(len(ds))
        draws = forced_draws(tables, rows, M, rng)
        want, _ = E.assemble_batch(tables, ds.size, rows, draws, M, augment)
        got = rset.assemble(dev_ints(rows, dev), tuple(torch.from_numpy(d).to(dev) for d in draws), M, augment)
        check_batch(got, want, augment, f"{name} M={M}")
        assert tuple(got[1].shape) == (len(rows), 1, 3)
    if not augment:
        return
    # the listed shifts under all four quarter turns: u = z_off + z, exact for the rows whose z is a multiple of 1/8
    z = tables["row_pos"][:, 2].astype(np.float64)
    exact = np.flatnonzero(z * 8 == np.round(z * 8)) if name == "f16" else np.arange(4)
    assert len(exact) >= 4
    rows = np.array([exact[(i // 4) % len(exact)] for i in range(4 * len(Z_OFFS))])
    z_offs = np.repeat(Z_OFFS, 4)
    draws = forced_draws(tables, rows, 7, rng, z_offs)
    assert sorted(set(draws[0].tolist())) == [0, 1, 2, 3]
    want, oks = E.assemble_batch(tables, ds.size, rows, draws, 7, True)
    if name == "f16":
        assert np.array_equal(draws[1] - z[rows], z_offs)                        # the shifts arrive exactly
        assert [int(ok.any(axis=(0, 1)).sum()) for ok in oks[::4]] == [40, 34, 33, 32, 6, 1, 0, 0, 36]      # source planes in range
    got = rset.assemble(dev_ints(rows, dev), tuple(torch.from_numpy(d).to(dev) for d in draws), 7, True)
    check_batch(got, want, True, f"{name} forced shifts")


@pytest.mark.parametrize("augment", [False, True], ids=["plain", "augment"])
def test_batch_of_33_equals_its_single_items_and_leaves_the_set_untouched(sets, augment):
    ds, rset, tables = sets["f16"]
    dev = rset.device
    before = {k: v.clone() for k, v in rset.tables.items()}
    rows = dev_ints(np.random.default_rng(23).permutation(len(ds))[:33], dev)
    ordinals = dev_ints(np.arange(33) * 3 + 1, dev)
    M = 300
    draws = rset.draw(ordinals, 2, 77, rows, M)
    batch = flat(rset.assemble(rows, draws, M, augment))
    for b in range(33):
        d1 = rset.draw(ordinals[b:b + 1], 2, 77, rows[b:b + 1], M)
        for a, c in zip(d1, draws):
            assert torch.equal(a, c[b:b + 1])
        one = flat(rset.assemble(rows[b:b + 1], d1, M, augment))
        for k in batch:
            assert np.array_equal(bits(one[k]), bits(batch[k][b:b + 1])), (k, b)
    again = flat(rset.assemble(rows, draws, M, augment))
    assert all(np.array_equal(bits(again[k]), bits(batch[k])) for k in batch)          # equal input, equal bytes
    for k, v in before.items():
        assert torch.equal(v, rset.tables[k]), k
        assert np.array_equal(v.cpu().numpy(), tables[k]), k


@pytest.mark.parametrize("drop_last", [False, True])
def test_iterator_epochs(sets, drop_last):
    ds, rset, tables = sets["sizes"]
    assert len(rset) == 40 and rset.num_point_occ == 64
    it = resident.ResidentBatches(rset, 32, seed=5, drop_last=drop_last)
    assert it.augment is True and len(it) == (1 if drop_last else 2)
    hb = ds.batch([0, 1], rng=np.random.default_rng(0))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    host = dataset.network_inputs((t(hb[0]), tuple(t(v) for v in hb[1]), t(hb[2]), t(hb[3]), t(hb[4])))
    epochs = []
    for epoch in (1, 2):
        batches = list(it)
        assert it.epoch == epoch and [b[0].shape[0] for b in batches] == ([32] if drop_last else [32, 8])
        order = resident.epoch_order(np.arange(40), 5, epoch)[1]
        for k, batch in enumerate(batches):
            x, pos, pos_occ, y = batch
            B = x.shape[0]
            for g, h in zip((x, pos, pos_occ) + y, host[:3] + host[3]):
                assert g.is_cuda and g.dtype == h.dtype == torch.float32 and tuple(g.shape[1:]) == tuple(h.shape[1:]), (g.shape, h.shape)
            # every row once: the un-augmented width and label identify the rows, and the epoch's order names them
            rows = order[32 * k:32 * k + B]
            assert np.array_equal(y[0].cpu().numpy(), tables["row_label"][rows])
            assert np.array_equal(y[2].cpu().numpy(), tables["row_width"][rows] / np.float32(ds.size))
        seen = np.concatenate([order[32 * k:32 * k + b[0].shape[0]] for k, b in enumerate(batches)])
        assert len(set(seen.tolist())) == len(seen) == (32 if drop_last else 40)
        epochs.append(batches)
    assert not torch.equal(epochs[0][0][0], epochs[1][0][0]) and not torch.equal(epochs[0][0][2], epochs[1][0][2])
    # a second iterator with the same seed repeats the bytes
    again = resident.ResidentBatches(rset, 32, seed=5, drop_last=drop_last)
    for batches in epochs:
        for a, b in zip(list(again), batches):
            fa, fb = flat(a), flat(b)
            assert all(torch.equal(fa[k], fb[k]) for k in fa)
    # ranks split an epoch; an item's bytes do not depend on the rank or the batch size
    whole = flat(next(iter(resident.ResidentBatches(rset, 40, seed=9))))
    order = resident.epoch_order(np.arange(40), 9, 1)[1]
    for rank in range(3):
        part = flat(next(iter(resident.ResidentBatches(rset, 40, seed=9, rank=rank, world=3))))
        assert all(torch.equal(part[k], whole[k][rank::3]) for k in whole)
    sub = resident.ResidentBatches(rset, 4, seed=9, indices=[7, 3, 11], augment=False)
    (only,) = list(sub)
    assert sorted(only[3][2].tolist()) == sorted((tables["row_width"][[7, 3, 11]] / np.float32(ds.size)).tolist())


def test_guards(sets, tmp_path):
    ds, rset, tables = sets["f32"]
    assert rset.nbytes == sum(v.nbytes for v in tables.values()) == sum(t.numel() * t.element_size() for t in rset.tables.values())
    torch.cuda.synchronize()
    allocated = torch.cuda.memory_allocated()
    with pytest.raises(_capi.GigaHipError, match="bytes"):
        resident.ResidentTrainingSet(ds, max_bytes=rset.nbytes - 1)
    assert torch.cuda.memory_allocated() == allocated                            # raised before any device allocation
    assert resident.ResidentTrainingSet(ds, max_bytes=rset.nbytes).nbytes == rset.nbytes
    for case in ("mixed", "shape"):
        root, raw = str(tmp_path / case / "data"), str(tmp_path / case / "raw")
        E.write_set(root, raw, [[5], [7, 3]], np.float32, grasps_per_scene=2, seed=4, res=20 if case == "shape" else 40)
        if case == "mixed":
            np.savez(raw + "/occ/w04_0001/0001.npz", points=np.zeros((3, 3), np.float16), occ=np.zeros(3, bool))
        with pytest.raises(ValueError):
            resident.ResidentTrainingSet(GraspOccDataset(root, raw))
    assert torch.cuda.memory_allocated() == allocated
    # CPU tensors raise, as everywhere else in the package
    rows = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(_capi.GigaHipError):
        rset.draw(rows, 0, 0, rows, 4)
    draws = rset.draw(rows.to(rset.device), 0, 0, rows.to(rset.device), 4)
    with pytest.raises(_capi.GigaHipError):
        rset.assemble(rows, draws, 4, True)
    with pytest.raises(_capi.GigaHipError):
        rset.assemble(rows.to(rset.device), (draws[0], draws[1].cpu(), draws[2], draws[3]), 4, True)
    with pytest.raises(ValueError):
        rset.assemble(rows.to(rset.device), draws, 5, True)                      # index is (B, 4)


def test_training_step_on_a_yielded_batch(sets, sd7):
    """one fp32 step of giga -- forward, giga_loss, backward -- on a yielded batch: finite losses, and the outputs of the same
    step on the same tensors passed in by hand (copies made through the host), so the yield is in the step's input form"""
    ds, rset, tables = sets["f16"]
    dev = rset.device
    x, pos, pos_occ, y = next(iter(resident.ResidentBatches(rset, 8, seed=1)))
    net = networks.get_network("giga"); net.load_state_dict(sd7); net = net.to(dev).train()

    def step(x, pos, pos_occ, y):
        net.zero_grad(set_to_none=True)
        out = net(x, pos, p_tsdf=pos_occ)
        loss, parts = giga_loss(out, y)
        loss.backward()
        return out, loss, parts, [p.grad.clone() for p in net.parameters()]

    out, loss, parts, grads = step(x, pos, pos_occ, y)
    assert torch.isfinite(loss).item() and all(torch.isfinite(torch.as_tensor(v)).all().item() for v in parts.values())
    assert all(torch.isfinite(g).all().item() for g in grads) and any(g.abs().max().item() > 0 for g in grads)
    by_hand = lambda t: torch.from_numpy(t.cpu().numpy().copy()).to(dev)  # noqa: E731
    out2, loss2, parts2, grads2 = step(by_hand(x), by_hand(pos), by_hand(pos_occ), tuple(by_hand(t) for t in y))
    assert all(torch.equal(a, b) for a, b in zip(out, out2)) and torch.equal(loss, loss2)
    for g, h in zip(grads, grads2):                          # (the bound tests/test_gpu_training.py holds a repeated backward to)
        assert (g - h).abs().max().item() <= 2e-3 * g.abs().max().item() + 1e-6
