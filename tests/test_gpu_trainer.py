"""GPU tests of the training loop (giga_amd.trainer, giga_train_loss_metrics): the accumulator kernel against the numpy
restatement (tests/trainer_emu.py), `giga_loss(..., metrics=m)` against the plain call, the Trainer end to end against a float64
recomputation from the run's own step tensors, resuming, and the host synchronisations of the batch loop."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import trainer_emu as E
from giga_amd import _capi, networks, resident, synth, trainer, weights
from giga_amd.dataset import GraspOccDataset
from giga_amd.optim import FlatAdam
from giga_amd.training import giga_loss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINELS = {7: 0x0123456789ABCDEF, 13: 0x1111, 14: -5, 15: 0x7FFFFFFFFFFFFFFF}          # reserved words: left as found


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype in (np.float64, np.int64) else a


def loss_inputs(B, M, rng, qual=None, label=None):
    """head outputs and labels of one batch in the loss's call shape, as device tensors"""
    rot = rng.standard_normal((B, 1, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    rot_t = rng.standard_normal((B, 2, 4)).astype(np.float32)
    rot_t /= np.linalg.norm(rot_t, axis=-1, keepdims=True)
    host = [E.edge_quals(B, rng).reshape(B, 1) if qual is None else np.asarray(qual, np.float32).reshape(B, 1), rot,
            rng.uniform(0, 1, (B, 1)).astype(np.float32), rng.standard_normal((B, M)).astype(np.float32) * 3,
            (rng.random(B) < 0.5).astype(np.float32) if label is None else np.asarray(label, np.float32).reshape(B), rot_t,
            rng.uniform(0, 1, B).astype(np.float32), (rng.random((B, M)) < 0.3).astype(np.float32)]
    return [torch.from_numpy(a).to(DEV) for a in host]


def raw_loss(args, acc=None):
    """giga_train_loss / giga_train_loss_metrics through the C ABI -> (losses [5], scene_losses [B][5])"""
    L = _capi.lib()
    B, M = args[3].shape
    losses, scene = torch.full((5,), -7.0, device=DEV), torch.full((B, 5), -7.0, device=DEV)
    ptrs = [_capi.ptr(t) for t in args]
    with torch.cuda.device(args[0].device):
        if acc is None:
            _capi.check(L.giga_train_loss(*ptrs, B, M, _capi.ptr(losses), _capi.ptr(scene), _capi.stream_ptr(DEV)), "giga_train_loss")
        else:
            _capi.check(L.giga_train_loss_metrics(*ptrs, B, M, _capi.ptr(losses), _capi.ptr(scene), _capi.ptr(acc),
                                                  _capi.stream_ptr(DEV)), "giga_train_loss_metrics")
    return losses, scene


def set_sentinels(m):
    for i, v in SENTINELS.items():
        m.acc[i] = v


@pytest.mark.parametrize("M", [0, 1, 7, 64])
def test_accumulator_equals_the_emulation(M):
    m = trainer.TrainMetrics(DEV)
    assert m.acc.dtype == torch.int64 and m.acc.numel() * 8 == _capi.TRAIN_METRICS_BYTES and m.acc.data_ptr() % 8 == 0
    for B in (1, 3, 63, 64, 65, 256, 257, 1000):
        rng = np.random.default_rng([31, M, B])
        set_sentinels(m)
        m.acc[:7] = 5
        m.reset()
        assert not m.words().any()                           # after reset() every word is zero
        set_sentinels(m)
        want = m.words().view(np.uint64)
        seen = set()
        for call in range(3):                                # three consecutive calls into one accumulator
            args = loss_inputs(B, M, rng)
            seen |= set(bits(args[0]).reshape(-1).tolist())
            plain = raw_loss(args)
            got = raw_loss(args, m.acc)
            for what, a, b in zip(("losses", "scene_losses"), got, plain):
                assert np.array_equal(bits(a), bits(b)), (what, B, M, call)
            want = E.update(want, args[0].cpu().numpy(), args[4].cpu().numpy(), plain[0].cpu().numpy())
        have = m.words().view(np.uint64)
        assert have[:7].tolist() == want[:7].tolist(), (B, M)                    # the seven counts
        assert have[0] == 3 and have[1] == 3 * B and have[6] == 0
        assert np.array_equal(have[8:13], want[8:13]), (B, M, have.view(np.float64)[8:13], want.view(np.float64)[8:13])
        assert [int(v) for v in have.view(np.int64)[[7, 13, 14, 15]]] == list(SENTINELS.values())       # the reserved words
        if B >= 5:                                           # 0, 1, 0.5 and its two neighbours were all there
            half = np.float32(0.5)
            edges = np.array([0, 1, half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))], np.float32)
            assert set(edges.view(np.uint32).tolist()) <= seen
        assert m.compute() == E.finalize(want)
    m.reset()
    assert not m.words().any()


def test_invalid_scenes_land_in_invalid_only():
    rng = np.random.default_rng(32)
    B, M = 70, 7
    for bad_q, bad_y in ((np.nan, None), (1.5, None), (None, 0.3), (-0.25, None), (None, 2.0)):
        qual, label = E.edge_quals(B, rng), (rng.random(B) < 0.5).astype(np.float32)
        where = [2, 66]                                      # one in each wave of the first round
        for i in where:
            if bad_q is not None:
                qual[i] = bad_q
            if bad_y is not None:
                label[i] = bad_y
        good = np.ones(B, bool)
        good[where] = False
        m = trainer.TrainMetrics(DEV)
        args = loss_inputs(B, M, rng, qual=qual, label=label)
        losses, _ = raw_loss(args, m.acc)
        have = m.words().view(np.uint64)
        want = E.update(np.zeros(16, np.uint64), qual, label, losses.cpu().numpy())
        assert have[:7].tolist() == want[:7].tolist()
        only_good = E.update(np.zeros(16, np.uint64), qual[good], label[good], np.zeros(5, np.float32))
        assert have[1:6].tolist() == only_good[1:6].tolist() and have[6] == 2 and have[0] == 1
        with pytest.raises(ValueError, match="2 scenes"):
            m.compute()


@pytest.mark.parametrize("M", [0, 64])
def test_giga_loss_with_metrics_equals_the_plain_call(M):
    rng = np.random.default_rng([33, M])
    B = 33
    args = loss_inputs(B, M, rng)
    m = trainer.TrainMetrics(DEV)

    def run(metrics):
        out = [t.clone().requires_grad_(True) for t in args[:4]]
        loss, d = giga_loss(tuple(out), tuple(args[4:]), metrics=metrics)
        (loss * 1.75).backward()
        return loss, d, [t.grad for t in out]

    loss0, d0, g0 = run(None)
    assert not m.words().any()
    loss1, d1, g1 = run(m)
    assert np.array_equal(bits(loss0), bits(loss1)) and list(d0) == list(d1)
    assert all(np.array_equal(bits(d0[k]), bits(d1[k])) for k in d0)
    for a, b in zip(g0, g1):
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b))
    w = m.words().view(np.uint64)
    want = E.update(np.zeros(16, np.uint64), args[0].cpu().numpy(), args[4].cpu().numpy(),
                    [d1[k].item() for k in E.LOSS_ORDER])
    assert np.array_equal(w, want)
    # an empty batch leaves the accumulator as it was
    empty = [t[:0] for t in args]
    loss, d = giga_loss(tuple(empty[:4]), tuple(empty[4:]), metrics=m)
    assert torch.isnan(loss).item() and np.array_equal(m.words().view(np.uint64), w)
    with pytest.raises(ValueError):
        giga_loss(tuple(args[:4]), tuple(args[4:]), metrics=type("M", (), {"acc": torch.zeros(8, dtype=torch.int64, device=DEV)})())


# ---------------------------------------------------------------------------------------------------------------- Trainer
@pytest.fixture(scope="module")
def rset(tmp_path_factory):
    base = tmp_path_factory.mktemp("trainer")
    root, raw = str(base / "data"), str(base / "raw")
    assert synth.write_training_set(root, raw, n_scenes=6, grasps_per_scene=5) == 30
    return resident.ResidentTrainingSet(GraspOccDataset(root, raw, num_point_occ=64, augment=True), device=DEV)


def make_net(net_name, seed=7):
    net = networks.get_network(net_name)
    net.load_state_dict(weights.make_state_dict(seed, with_tsdf=net_name != "giga_aff"))
    return net.to(DEV)


def make_batches(rset, seed=3, val_split=0.2):
    tr, va = trainer.train_val_split(len(rset), val_split, seed)
    return (resident.ResidentBatches(rset, 4, shuffle=True, seed=seed, drop_last=True, indices=tr),
            resident.ResidentBatches(rset, 4, shuffle=False, seed=seed, drop_last=True, indices=va))


class StepLog:
    """the on_step hook of the tests: keeps every step's quality outputs, labels and loss means (copies, made on the device)"""

    def __init__(self):
        self.steps = []

    def __call__(self, tr, batch, out, loss_dict):
        self.steps.append((tr.phase, tr.epoch, out[0].detach().clone(), batch[3][0].clone(), tuple(out[3].shape),
                           torch.stack([loss_dict[k] for k in E.LOSS_ORDER]).clone()))

    def metrics(self, phase, epoch):
        """the metrics of the steps of `phase` seen while `epoch` epochs were complete, recomputed in float64"""
        w, n = np.zeros(16, np.uint64), 0
        for ph, ep, qual, label, _, losses in self.steps:
            if (ph, ep) == (phase, epoch):
                w = E.update(w, qual.cpu().numpy(), label.cpu().numpy(), losses.cpu().numpy())
                n += 1
        return E.finalize(w), n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("net_name", ["giga", "giga_aff"])
def test_trainer_end_to_end(rset, tmp_path, net_name, precision, capsys):
    net = make_net(net_name)
    train_b, val_b = make_batches(rset)
    assert len(train_b) == 6 and len(val_b) == 1
    log = StepLog()
    logdir = tmp_path / "run"
    tr = trainer.Trainer(net, train_b, val_b, lr=2e-4, net_name=net_name, logdir=logdir, precision=precision, on_step=log)
    records = tr.run(2)
    assert [r["epoch"] for r in records] == [1, 2] and [r["iteration"] for r in records] == [6, 12]
    assert int(tr.metrics.words()[0]) == len(train_b) == 6                       # batches
    for r in records:
        # train steps of epoch e run while e - 1 epochs are complete, its validation after e
        want, n = log.metrics("train", r["epoch"] - 1)
        assert n == 6 and r["train"] == want, (r["train"], want)
        want, n = log.metrics("val", r["epoch"])
        assert n == 1 and r["val"] == want, (r["val"], want)
        assert list(r["train"]) == list(E.KEYS) and all(np.isfinite(v) for v in r["train"].values())
    M = 0 if net_name == "giga_aff" else 64
    assert all(s[4] == (4, M) for s in log.steps)
    out = capsys.readouterr().out.splitlines()
    assert [line.split()[0] for line in out if line.startswith(("Train", "Val"))] == ["Train", "Val"] * 2
    assert out[0] == "Train" + "".join(f" {k}: {v:.4f}" for k, v in records[0]["train"].items())
    # the files
    lines = open(logdir / "metrics.jsonl").read().splitlines()
    assert len(lines) == 2 and [json.loads(line) for line in lines] == records
    names = sorted(os.listdir(logdir))
    best = [n for n in names if n.startswith("best_")]
    assert len(best) == 1 and f"vgn_{net_name}_12.pt" in names and len(names) == 4 and "trainer_state.pt" in names
    assert best[0] == f"best_vgn_{net_name}_val_acc={max(r['val']['accuracy'] for r in records):.4f}.pt"
    loaded = networks.load_network(str(logdir / f"vgn_{net_name}_12.pt"), torch.device(DEV), net_name)
    sd = net.state_dict()
    assert list(loaded.state_dict()) == list(sd) == list(weights.giga_param_shapes(with_tsdf=net_name != "giga_aff"))
    assert all(np.array_equal(bits(v), bits(sd[k])) for k, v in loaded.state_dict().items())
    # validation leaves every parameter byte unchanged and the net in training mode
    flat = net.flatten_parameters()[0]
    before, steps = flat.detach().clone(), len(log.steps)
    again = tr.validate()
    assert again is not None and net.training and np.array_equal(bits(before), bits(flat))
    assert len(log.steps) == steps + 1 and tr.iteration == 12
    assert not torch.equal(before.cpu(), torch.cat([v.reshape(-1) for v in weights.make_state_dict(7, with_tsdf=M > 0).values()]))


def test_empty_validation_is_skipped(rset, tmp_path):
    net = make_net("giga")
    train_b, _ = make_batches(rset)
    val_b = resident.ResidentBatches(rset, 4, shuffle=False, drop_last=True, indices=[1, 2, 3])
    assert len(val_b) == 0
    tr = trainer.Trainer(net, train_b, val_b, logdir=tmp_path / "run", quiet=True)
    (record,) = tr.run(1)
    assert record["val"] is None and record["train"] is not None and tr.best_score is None
    assert sorted(os.listdir(tmp_path / "run")) == ["metrics.jsonl", "trainer_state.pt", "vgn_giga_6.pt"]
    assert json.loads(open(tmp_path / "run" / "metrics.jsonl").read())["val"] is None
    with pytest.raises(ValueError, match="resume"):
        trainer.Trainer(make_net("giga"), train_b, val_b, logdir=tmp_path / "run")


def test_trainer_under_a_process_group(rset, tmp_path):
    """the group's code path in one process (a gloo group of one rank): parameters broadcast, the steps of an epoch agreed on
    beforehand, the gradient and the accumulator reduced, a validation share without a batch skipped by agreement"""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    try:
        net = make_net("giga")
        start = net.flatten_parameters()[0].detach().clone()
        train_b, val_b = make_batches(rset)
        none_b = resident.ResidentBatches(rset, 4, shuffle=False, drop_last=True, indices=[1, 2, 3])
        log = StepLog()
        tr = trainer.Trainer(net, train_b, none_b, group=dist.group.WORLD, logdir=tmp_path / "run", on_step=log, quiet=True)
        assert (tr.train_steps, tr.val_steps, tr.rank) == (6, 0, 0)
        assert np.array_equal(bits(start), bits(net.flatten_parameters()[0]))
        (record,) = tr.run(1)
        want, n = log.metrics("train", 0)
        assert n == 6 and record["train"] == want and record["val"] is None and tr.iteration == 6
        tr2 = trainer.Trainer(make_net("giga"), train_b, val_b, group=dist.group.WORLD, on_step=log, quiet=True)
        assert (tr2.train_steps, tr2.val_steps) == (6, 1)
        tr2.train_steps = 2                                  # what a rank with a larger share does: it stops with the others
        tr2.train_epoch()
        assert tr2.iteration == 2 and int(tr2.metrics.words()[0]) == 2 and tr2.validate() is not None
    finally:
        dist.destroy_process_group()


def test_resume(rset, tmp_path):
    logdir = tmp_path / "run"
    first = trainer.Trainer(make_net("giga"), *make_batches(rset), logdir=logdir, precision="bf16", quiet=True)
    first.run(1)
    second = trainer.Trainer(make_net("giga", seed=11), *make_batches(rset), logdir=logdir, precision="bf16", resume=True, quiet=True)
    assert (second.epoch, second.iteration) == (first.epoch, first.iteration) == (1, 6)
    assert second.best_score == first.best_score and first.best_score is not None
    p1, p2 = first.net.flatten_parameters()[0], second.net.flatten_parameters()[0]
    assert np.array_equal(bits(p1), bits(p2))
    s1, s2 = first.optimizer.state[p1], second.optimizer.state[p2]
    assert sorted(s1) == sorted(s2) == ["exp_avg", "exp_avg_sq", "step"]
    for k in ("exp_avg", "exp_avg_sq", "step"):
        assert s1[k].dtype == s2[k].dtype and s1[k].device == s2[k].device and np.array_equal(bits(s1[k]), bits(s2[k])), k
    assert float(s2["step"]) == 6.0
    assert first.optimizer.state_dict()["param_groups"] == second.optimizer.state_dict()["param_groups"]
    assert (second.train_batches.seed, second.train_batches.epoch) == (first.train_batches.seed, first.train_batches.epoch) == (3, 1)
    a, b = next(iter(first.train_batches)), next(iter(second.train_batches))    # the first batch of the next epoch
    for u, v in zip(a[:3] + a[3], b[:3] + b[3]):
        assert np.array_equal(bits(u), bits(v))
    # the resumed run goes on with the next epoch
    records = second.run(2)
    assert [r["epoch"] for r in records] == [2] and records[0]["iteration"] == 12
    assert len(open(logdir / "metrics.jsonl").read().splitlines()) == 2 and os.path.exists(logdir / "vgn_giga_12.pt")
    assert not os.path.exists(logdir / "vgn_giga_6.pt")


def test_command_line_trains_one_epoch(tmp_path, capsys):
    """`python -m giga_amd.train`'s main on a small set in the reference's layout, in this process"""
    from giga_amd import train
    root, raw, out = str(tmp_path / "data"), str(tmp_path / "raw"), tmp_path / "out"
    assert synth.write_training_set(root, raw, n_scenes=2, grasps_per_scene=10, occ_files=(1, 1), n_occ_points=4096, seed=5) == 20
    train.main(["--dataset", root, "--dataset_raw", raw, "--savedir", str(out), "--epochs", "1", "--batch-size", "4", "--val-split", "0.2",
                "--augment", "--precision", "bf16", "--seed", "2"])
    names = sorted(os.listdir(out))                          # 16 train rows: 4 steps; 4 validation rows: one batch
    assert "vgn_giga_4.pt" in names and "trainer_state.pt" in names and len([n for n in names if n.startswith("best_vgn_giga_val_acc=")]) == 1
    (record,) = [json.loads(line) for line in open(out / "metrics.jsonl")]
    assert record["epoch"] == 1 and record["iteration"] == 4 and list(record["train"]) == list(record["val"]) == list(E.KEYS)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("Namespace(") and [line.split()[0] for line in lines[1:]] == ["Train", "Val"]
    with pytest.raises(ValueError, match="resume"):          # the directory now holds checkpoints
        train.main(["--dataset", root, "--dataset_raw", raw, "--savedir", str(out), "--epochs", "1", "--batch-size", "4"])


def test_batch_loop_adds_no_host_waits(rset):
    """torch's synchronisation warnings inside the batch loop: the Trainer's against a bare loop over the same batches on the
    parent's pieces (net, giga_loss without metrics, backward, FlatAdam)"""
    net = make_net("giga")
    train_b, _ = make_batches(rset)
    counts = []

    def hook(tr, batch, out, loss_dict):
        counts.append(len(caught))

    tr = trainer.Trainer(net, train_b, precision="bf16", on_step=None)
    opt = FlatAdam(net.flatten_parameters(), lr=2e-4)

    def bare_epoch():
        net.train()
        for x, pos, pos_occ, y in train_b:
            opt.zero_grad(set_to_none=True)
            loss, _ = giga_loss(net(x, pos, p_tsdf=pos_occ), y)
            loss.backward()
            opt.step()

    tr.train_epoch()                                         # warm both: buffers, the optimiser's state
    bare_epoch()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            probe = torch.ones(1, device=DEV).item()         # the mode itself: a host read of a device value is reported
            assert probe == 1.0 and len(caught) >= 1, "this torch build does not report synchronisations on ROCm"
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            bare_epoch()
            bare = len(caught)
        tr.on_step = hook
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            tr.train_epoch()
            whole = len(caught)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(counts) == len(train_b) == 6
    print(f"synchronisation warnings: bare loop {bare}, Trainer's loop {counts[-1]} (whole epoch with the metrics copy {whole})")
    assert counts[-1] <= bare
