"""GPU tests of giga_geo's training half (giga_train_occ_loss*, giga_amd.training.geo_loss, the differentiable forward of
ConvolutionalOccupancyNetworkGeometry, giga_amd.trainer.GeoTrainer, giga_amd.train_geo): the loss kernels against the joint
loss's occupancy term bit for bit, the point accumulator against the numpy restatement (tests/geo_trainer_emu.py), the module's
training path against the autograd function on head set 8 that tests/test_gpu_backward_envelope.py holds to float64, the bf16
step against `giga`'s with silent grasp heads, the inference caches after a step, and the loop end to end."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import geo_trainer_emu as G
from giga_amd import _capi, networks, resident, synth, trainer, weights
from giga_amd.dataset import GraspOccDataset
from giga_amd.optim import FlatAdam
from giga_amd.training import GigaFunction, _TrainState, geo_loss

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEO_HEADS = ("decoder_tsdf",)
# words the occupancy loss leaves as found: the reserved ones and the sums of the three grasp losses (doubles 8-10)
SENTINELS = {7: 0x0123456789ABCDEF, 8: 0x3FF8000000000000, 9: -7, 10: 0x4004000000000000, 13: 0x1111, 14: -5, 15: 0x7FFFFFFFFFFFFFFF}


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype in (np.float64, np.int64) else a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------------ the loss kernels
def occ_loss(z, t, acc=None):
    """giga_train_occ_loss / giga_train_occ_loss_metrics through the C ABI -> (loss [1], scene_losses [B])"""
    L = _capi.lib()
    B, M = z.shape
    loss, scene = torch.full((1,), -7.0, device=DEV), torch.full((B,), -7.0, device=DEV)
    with torch.cuda.device(z.device):
        if acc is None:
            _capi.check(L.giga_train_occ_loss(_capi.ptr(z), _capi.ptr(t), B, M, _capi.ptr(loss), _capi.ptr(scene), _capi.stream_ptr(DEV)),
                        "giga_train_occ_loss")
        else:
            counts = torch.full((B, 6), -1, dtype=torch.int32, device=DEV)
            _capi.check(L.giga_train_occ_loss_metrics(_capi.ptr(z), _capi.ptr(t), B, M, _capi.ptr(loss), _capi.ptr(scene),
                                                      _capi.ptr(counts), _capi.ptr(acc), _capi.stream_ptr(DEV)),
                        "giga_train_occ_loss_metrics")
    return loss, scene


def occ_loss_backward(z, t, g):
    L = _capi.lib()
    B, M = z.shape
    docc = torch.full((B, M), -7.0, device=DEV)
    with torch.cuda.device(z.device):
        _capi.check(L.giga_train_occ_loss_backward(_capi.ptr(z), _capi.ptr(t), _capi.ptr(g), B, M, _capi.ptr(docc),
                                                   _capi.stream_ptr(DEV)), "giga_train_occ_loss_backward")
    return docc


def joint_loss(z, t, g, rng):
    """the joint objective's kernels on the same logits and targets (its other inputs: arbitrary valid values)
    -> (losses [5], scene_losses [B][5], docc)"""
    L = _capi.lib()
    B, M = z.shape
    rot = rng.standard_normal((B, 1, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
    rot_t = rng.standard_normal((B, 2, 4)).astype(np.float32)
    rot_t /= np.linalg.norm(rot_t, axis=-1, keepdims=True)
    args = [dev(rng.uniform(0.05, 0.95, (B, 1)).astype(np.float32)), dev(rot), dev(rng.uniform(0, 1, (B, 1)).astype(np.float32)), z,
            dev((rng.random(B) < 0.5).astype(np.float32)), dev(rot_t), dev(rng.uniform(0, 1, B).astype(np.float32)), t]
    ptrs = [_capi.ptr(a) for a in args]
    losses, scene = torch.empty(5, device=DEV), torch.empty((B, 5), device=DEV)
    dq, dr, dw, docc = (torch.empty(s, device=DEV) for s in ((B, 1), (B, 1, 4), (B, 1), (B, M)))
    with torch.cuda.device(z.device):
        _capi.check(L.giga_train_loss(*ptrs, B, M, _capi.ptr(losses), _capi.ptr(scene), _capi.stream_ptr(DEV)), "giga_train_loss")
        _capi.check(L.giga_train_loss_backward(*ptrs, _capi.ptr(g), B, M, _capi.ptr(dq), _capi.ptr(dr), _capi.ptr(dw), _capi.ptr(docc),
                                               _capi.stream_ptr(DEV)), "giga_train_loss_backward")
    return losses, scene, docc


@pytest.mark.parametrize("M", [1, 7, 64, 255, 256, 257, 300])
def test_occ_loss_equals_the_joint_loss_bit_for_bit(M):
    g = torch.full((1,), 3.0, device=DEV)
    for B in (1, 3, 5):
        rng = np.random.default_rng([41, M, B])
        z = dev(G.edge_logits((B, M), rng))
        t = dev((rng.random((B, M)) < 0.3).astype(np.float32))
        losses, scene5, docc5 = joint_loss(z, t, g, rng)
        loss, scene = occ_loss(z, t)
        assert torch.isfinite(loss).all() and loss.item() > 0
        assert np.array_equal(bits(loss), bits(losses[3:4])), (B, M, loss.item(), losses[3].item())
        assert np.array_equal(bits(scene), bits(scene5[:, 3].contiguous())), (B, M)
        docc = occ_loss_backward(z, t, g)
        assert np.array_equal(bits(docc), bits(docc5)), (B, M)
        m = trainer.TrainMetrics(DEV)
        loss_m, scene_m = occ_loss(z, t, m.acc)
        assert np.array_equal(bits(loss_m), bits(loss)) and np.array_equal(bits(scene_m), bits(scene)), (B, M)
        assert m.words()[0] == 1 and m.words()[1] == B * M


def test_geo_loss_against_torch_autograd():
    """geo_loss against fp32 torch autograd on the CPU of the reference's two lines (train_giga_geo.py:152-165), with the bounds
    tests/test_gpu_training.py::test_fused_loss_matches_reference_helpers_g11 holds giga_loss to"""
    rng = np.random.default_rng(42)
    B, M = 3, 300
    z = (rng.standard_normal((B, M)) * 3).astype(np.float32)
    z[:, :4] = np.float32([30.0, -30.0, 120.0, -120.0])      # saturated: ATen's clamped BCE arithmetic
    z[:, 4:8] = np.float32([30.0, -30.0, 120.0, -120.0])
    t = (rng.random((B, M)) < 0.3).astype(np.float32)
    t[:, :4], t[:, 4:8] = 1.0, 0.0
    a = dev(z).requires_grad_(True)
    loss, d = geo_loss(a, dev(t))
    assert list(d) == ["loss"] and np.array_equal(bits(d["loss"]), bits(loss)) and not d["loss"].requires_grad
    (3.0 * loss).backward()
    b = torch.from_numpy(z).requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy(torch.sigmoid(b), torch.from_numpy(t), reduction="none").mean(-1).mean()
    (3.0 * ref).backward()
    print(f"geo_loss {loss.item():.9g} reference {ref.item():.9g}")
    assert abs(loss.item() - ref.item()) <= 2e-6 * max(1.0, abs(ref.item()))
    scale = b.grad.abs().max().item()
    err = (a.grad.cpu() - b.grad).abs().max().item()
    print(f"gradient: max error {err:.3e}, scale {scale:.3e}")
    assert a.grad.shape == (B, M) and err <= 1e-5 * scale + 1e-9
    # shapes, devices and the empty batch
    with pytest.raises(ValueError):
        geo_loss(dev(z)[0], dev(t)[0])
    with pytest.raises(ValueError):
        geo_loss(dev(z), dev(t)[:, :-1])
    with pytest.raises(ValueError):
        geo_loss(dev(z)[:, :0], dev(t)[:, :0])
    with pytest.raises(_capi.GigaHipError):
        geo_loss(dev(z), torch.from_numpy(t))
    m = trainer.TrainMetrics(DEV)
    empty, de = geo_loss(dev(z)[:0].requires_grad_(True), dev(t)[:0], metrics=m)
    assert torch.isnan(empty).item() and torch.isnan(de["loss"]).item() and not m.words().any()
    with pytest.raises(ValueError):
        geo_loss(dev(z), dev(t), metrics=type("M", (), {"acc": torch.zeros(8, dtype=torch.int64, device=DEV)})())


# ------------------------------------------------------------------------------------------------------ the accumulator
@pytest.mark.parametrize("M", [1, 7, 64, 257])
def test_point_accumulator_equals_the_emulation(M):
    m = trainer.TrainMetrics(DEV)
    for B in (1, 3, 65, 200):
        rng = np.random.default_rng([43, M, B])
        m.reset()
        for i, v in SENTINELS.items():
            m.acc[i] = v
        want = m.words().view(np.uint64)
        seen = set()
        for call in range(2):                                # the second call starts from non-zero words
            z = G.edge_logits((B, M), rng)
            t = (rng.random((B, M)) < 0.4).astype(np.float32)
            seen |= set(z.view(np.uint32).reshape(-1).tolist())
            plain = occ_loss(dev(z), dev(t))
            got = occ_loss(dev(z), dev(t), m.acc)
            for what, a, b in zip(("loss", "scene_losses"), got, plain):
                assert np.array_equal(bits(a), bits(b)), (what, B, M, call)
            want = G.update(want, z, t, plain[0].cpu().numpy()[0])
        have = m.words().view(np.uint64)
        assert have.tolist() == want.tolist(), (B, M, have, want)                # all sixteen words
        assert have[0] == 2 and have[1] == 2 * B * M and have[6] == 0 and have[2] <= have[1]
        assert [int(v) for v in have.view(np.int64)[list(SENTINELS)]] == list(SENTINELS.values())
        assert have[11] == have[12] and have.view(np.float64)[11] > 0
        if B * M >= 8:                                       # +-0.0, +-1e-6, +-120 and +-inf were all there
            edges = np.array([0.0, -0.0, 1e-6, -1e-6, 120.0, -120.0, np.inf, -np.inf], np.float32)
            assert set(edges.view(np.uint32).tolist()) <= seen
        assert trainer.finalize_geo_metrics(m.words()) == G.finalize(want)


def test_invalid_points_land_in_invalid_only():
    rng = np.random.default_rng(44)
    B, M = 3, 300
    z = G.edge_logits((B, M), rng)
    t = (rng.random((B, M)) < 0.4).astype(np.float32)
    # one per wave of the first round, the ragged last round, and a scene of its own kind each
    nan_at, half_at, two_at = [(0, 2), (0, 70), (1, 299)], [(0, 130), (2, 256)], [(1, 200), (2, 44), (2, 299)]
    for b, i in nan_at:
        z[b, i] = np.nan
    for b, i in half_at:
        t[b, i] = 0.5
    for b, i in two_at:
        t[b, i] = 2.0
    bad = np.zeros((B, M), bool)
    for b, i in nan_at + half_at + two_at:
        bad[b, i] = True
    m = trainer.TrainMetrics(DEV)
    loss, _ = occ_loss(dev(z), dev(t), m.acc)
    have = m.words().view(np.uint64)
    want = G.update(np.zeros(16, np.uint64), z, t, loss.cpu().numpy()[0])
    assert have[:7].tolist() == want[:7].tolist()
    only_good = G.update(np.zeros(16, np.uint64), z[~bad], t[~bad], 0.0)
    assert have[1:6].tolist() == only_good[1:6].tolist() and have[6] == 8 and have[0] == 1 and have[1] == B * M - 8
    with pytest.raises(ValueError, match="8 points"):
        trainer.finalize_geo_metrics(m.words())
    # through geo_loss, and without a NaN in the loss: the counts are there, the finalisation refuses them
    z[np.isnan(z)] = 1.0
    m.reset()
    loss, _ = geo_loss(dev(z), dev(t), metrics=m)
    assert m.words()[6] == 5 and m.words()[1] == B * M - 5
    with pytest.raises(ValueError, match="5 points"):
        trainer.finalize_geo_metrics(m.words())


# ------------------------------------------------------------------------------------------------------ the module's forward
def geo_net(seed=11):
    net = networks.get_network("giga_geo")
    net.load_state_dict(weights.make_state_dict(seed, heads=GEO_HEADS))
    return net.to(DEV)


def scene_inputs(B, M, seed=21):
    x = torch.from_numpy(synth.tsdf_batch(seed, B)).to(DEV)
    pos_occ = torch.from_numpy(synth.query_points(seed + 1, B, M, stream=7, half_width=0.45)).to(DEV)
    R = torch.randn((B, M), generator=torch.Generator().manual_seed(seed)).to(DEV)
    return x, pos_occ, R


def check_against_runs(runs, other, names, what):
    """`runs`: the same tensors from repeated runs of one path; `other`: from the path under test.  A tensor that is equal in all
    runs must be equal in `other`; any other (fp32 atomics) must stay within 4x the run-to-run spread -> how many were equal"""
    n_det = 0
    for i, name in enumerate(names):
        a = runs[0][i]
        assert a.shape == other[i].shape, (what, name)
        if all(torch.equal(a, r[i]) for r in runs[1:]):
            n_det += 1
            assert torch.equal(a, other[i]), (what, name)
        else:
            spread = max((a - r[i]).abs().max().item() for r in runs[1:])
            assert (a - other[i]).abs().max().item() <= 4 * spread + 1e-7 * a.abs().max().item(), (what, name)
    return n_det


def test_module_training_path_equals_the_autograd_function():
    B, M = 3, 300
    x, pos_occ, R = scene_inputs(B, M)
    net = geo_net()
    names = {id(q): n for n, q in net.named_parameters()}
    keys = [names[id(q)] for q in net._ordered_params()]
    assert keys == list(weights.giga_param_shapes(heads=GEO_HEADS))
    no_grasp = torch.empty((B, 0, 3), device=DEV)
    held = []
    for _ in range(8):
        params = [q.detach().clone().requires_grad_(True) for q in net._ordered_params()]
        (occ,) = GigaFunction.apply(_TrainState(8, torch.device(DEV)), x, no_grasp, pos_occ, *params)
        (occ * R).sum().backward()
        held.append([occ.detach()] + [q.grad for q in params])
    assert all(np.array_equal(bits(held[0][0]), bits(h[0])) for h in held[1:])  # the forward has no atomics

    def module_run(net):
        net.train()
        logits = net(x, None, p_tsdf=pos_occ)
        assert logits.shape == (B, M) and logits.requires_grad
        (logits * R).sum().backward()
        return logits.detach()

    logits = module_run(net)
    separate = [logits] + [q.grad for q in net._ordered_params()]
    n_det = check_against_runs(held, separate, ["logits"] + keys, "separate parameters")
    assert n_det > 1 and np.array_equal(bits(logits), bits(held[0][0]))
    flat_net = geo_net()
    (flat,) = flat_net.flatten_parameters()
    logits = module_run(flat_net)
    assert flat.grad is not None and all(q.grad is None for q in flat_net._ordered_params())
    views, at = [], 0
    for q in flat_net._ordered_params():
        views.append(flat.grad[at:at + q.numel()].view(q.shape))
        at += q.numel()
    assert at == flat.numel()
    assert check_against_runs(held, [logits] + views, ["logits"] + keys, "flattened") == n_det
    # under no_grad and in eval mode with frozen parameters the call is the inference path
    with torch.no_grad():
        assert not net(x, None, p_tsdf=pos_occ).requires_grad
    with pytest.raises(ValueError):
        net(x, None, p_tsdf=pos_occ[:, :0])


@pytest.mark.parametrize("M", [64, 300])
def test_bf16_step_on_the_occupancy_head_alone(M):
    """set_train_precision("bf16") on head set 8 alone, against `giga` in bf16 on the same encoder and decoder_tsdf weights whose
    three grasp heads get all-zero upstream gradients (they then add exact zeros to the plane gradients)"""
    B = 2
    x, pos_occ, R = scene_inputs(B, M, seed=31)
    pos = torch.from_numpy(synth.query_points(33, B, 1, stream=7, half_width=0.45)).to(DEV)
    giga = networks.get_network("giga")
    giga.load_state_dict(weights.make_state_dict(11))
    giga = giga.to(DEV).train().set_train_precision("bf16")
    geo = geo_net(11).train().set_train_precision("bf16")
    sd_a, sd_b = giga.state_dict(), geo.state_dict()
    assert all(np.array_equal(bits(v), bits(sd_a[k])) for k, v in sd_b.items())
    keys = list(sd_b)
    runs = []
    for _ in range(8):
        giga.zero_grad(set_to_none=True)
        out = giga(x, pos, p_tsdf=pos_occ)
        (out[3] * R).sum().backward()
        g = {n: q.grad for n, q in giga.named_parameters()}
        assert all(not g[n].any() for n in g if n.startswith(("decoder_qual", "decoder_rot", "decoder_width")))
        runs.append([out[3].detach()] + [g[k] for k in keys])
    logits = geo(x, None, p_tsdf=pos_occ)
    (logits * R).sum().backward()
    g = {n: q.grad for n, q in geo.named_parameters()}
    assert np.array_equal(bits(logits), bits(runs[0][0]))
    assert all(torch.isfinite(g[k]).all() for k in keys) and any(g[k].any() for k in keys if k.startswith("encoder"))
    check_against_runs(runs, [logits.detach()] + [g[k] for k in keys], ["logits"] + keys, f"bf16 M={M}")


# ---------------------------------------------------------------------------------------------------------------- GeoTrainer
@pytest.fixture(scope="module")
def rset(tmp_path_factory):
    base = tmp_path_factory.mktemp("geo_trainer")
    root, raw = str(base / "data"), str(base / "raw")
    assert synth.write_training_set(root, raw, n_scenes=6, grasps_per_scene=5) == 30
    return resident.ResidentTrainingSet(GraspOccDataset(root, raw, num_point_occ=64, augment=True), device=DEV)


def make_batches(rset, seed=3, val_split=0.2):
    tr, va = trainer.train_val_split(len(rset), val_split, seed)
    return (resident.ResidentBatches(rset, 4, shuffle=True, seed=seed, drop_last=True, indices=tr),
            resident.ResidentBatches(rset, 4, shuffle=False, seed=seed, drop_last=True, indices=va))


class StepLog:
    """the on_step hook of the tests: keeps every step's logits, targets and loss (copies, made on the device)"""

    def __init__(self):
        self.steps = []

    def __call__(self, tr, batch, out, loss_dict):
        assert out[:3] == (None, None, None) and list(loss_dict) == ["loss"]
        self.steps.append((tr.phase, tr.epoch, out[3].detach().clone(), batch[3][3].clone(), loss_dict["loss"].clone()))

    def metrics(self, phase, epoch):
        """the metrics of the steps of `phase` seen while `epoch` epochs were complete, recomputed by the emulation"""
        w, n = np.zeros(16, np.uint64), 0
        for ph, ep, logits, target, loss in self.steps:
            if (ph, ep) == (phase, epoch):
                # (a network's logits may fall where the emulation's rule does not reach: numpy's float32 sigmoid there)
                w = G.update(w, logits.cpu().numpy(), target.cpu().numpy(), loss.cpu().numpy(), band="float32")
                n += 1
        return G.finalize(w), n


def test_stale_weights_after_a_step(rset):
    net = geo_net(7)
    batch = next(iter(make_batches(rset)[0]))
    x, _, pos_occ, _ = batch

    def infer(net):
        net.eval()
        with torch.no_grad():
            whole = net(x, None, p_tsdf=pos_occ)
            pieces = net.decode_occ(pos_occ, net.encode_inputs(x)).logits
            geo = net.infer_geo(x, pos_occ)
        return whole, pieces, geo

    tr = trainer.GeoTrainer(net, [batch])                    # (flattens the parameters, which drops the caches: before they fill)
    before = infer(net)                                      # packs the blobs the step must not leave in use
    # the step runs with grad enabled, which is all the training path asks; the module stays in eval mode, so that no train() /
    # eval() switch drops the caches on the way, and FlatAdam bumps no version counter: the step's own mark has to
    tr.train_step(batch)
    assert not net.training
    after = infer(net)
    fresh = networks.get_network("giga_geo")
    fresh.load_state_dict({k: v.detach().cpu().clone() for k, v in net.state_dict().items()})
    want = infer(fresh.to(DEV))
    for a, b, c in zip(after, want, before):
        assert np.array_equal(bits(a), bits(b))
        assert not np.array_equal(bits(a), bits(c))
    # the point gradients read the new weights too
    p = pos_occ.clone().requires_grad_(True)
    for q in net.parameters():
        q.requires_grad_(False)
    net.flatten_parameters()[0].requires_grad_(False)
    net(x, None, p_tsdf=p).sum().backward()
    assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max().item() > 0


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_geo_trainer_end_to_end(rset, tmp_path, precision, capsys):
    net = geo_net(7)
    train_b, val_b = make_batches(rset)
    assert len(train_b) == 6 and len(val_b) == 1
    log = StepLog()
    logdir = tmp_path / "run"
    tr = trainer.GeoTrainer(net, train_b, val_b, lr=2e-4, logdir=logdir, precision=precision, on_step=log)
    assert tr.net_name == "giga_geo"
    records = tr.run(2)
    assert [r["epoch"] for r in records] == [1, 2] and [r["iteration"] for r in records] == [6, 12]
    w = tr.metrics.words()
    assert int(w[0]) == len(train_b) == 6 and int(w[1]) == 6 * 4 * 64          # batches; examples, in points
    for r in records:
        # train steps of epoch e run while e - 1 epochs are complete, its validation after e
        want, n = log.metrics("train", r["epoch"] - 1)
        assert n == 6 and r["train"] == want, (r["train"], want)
        want, n = log.metrics("val", r["epoch"])
        assert n == 1 and r["val"] == want, (r["val"], want)
        assert list(r["train"]) == list(r["val"]) == list(G.KEYS) and all(np.isfinite(v) for v in r["train"].values())
    assert all(tuple(s[2].shape) == (4, 64) == tuple(s[3].shape) for s in log.steps)
    out = capsys.readouterr().out.splitlines()
    assert [line.split()[0] for line in out if line.startswith(("Train", "Val"))] == ["Train", "Val"] * 2
    assert out[0] == "Train" + "".join(f" {k}: {v:.4f}" for k, v in records[0]["train"].items())
    assert out[1] == "Val" + "".join(f" {k}: {v:.4f}" for k, v in records[0]["val"].items())
    assert out[0].split()[1::2] == ["loss:", "occ_accuracy:", "occ_precision:", "occ_recall:"]
    # the files
    lines = open(logdir / "metrics.jsonl").read().splitlines()
    assert len(lines) == 2 and [json.loads(line) for line in lines] == records
    names = sorted(os.listdir(logdir))
    best = [n for n in names if n.startswith("best_")]
    assert len(best) == 1 and "vgn_giga_geo_12.pt" in names and len(names) == 4 and "trainer_state.pt" in names
    assert best[0] == f"best_vgn_giga_geo_val_acc={max(r['val']['occ_accuracy'] for r in records):.4f}.pt"
    loaded = networks.load_network(str(logdir / "vgn_giga_geo_12.pt"), torch.device(DEV), "giga_geo")
    sd = net.state_dict()
    assert list(loaded.state_dict()) == list(sd) == list(weights.giga_param_shapes(heads=GEO_HEADS))
    assert all(np.array_equal(bits(v), bits(sd[k])) for k, v in loaded.state_dict().items())
    # validation leaves every parameter byte unchanged and the net in training mode
    flat = net.flatten_parameters()[0]
    before, steps = flat.detach().clone(), len(log.steps)
    again = tr.validate()
    assert again is not None and net.training and np.array_equal(bits(before), bits(flat))
    assert len(log.steps) == steps + 1 and tr.iteration == 12
    assert not torch.equal(before.cpu(), torch.cat([v.reshape(-1) for v in weights.make_state_dict(7, heads=GEO_HEADS).values()]))


def test_geo_resume(rset, tmp_path):
    logdir = tmp_path / "run"
    first = trainer.GeoTrainer(geo_net(7), *make_batches(rset), logdir=logdir, precision="bf16", quiet=True)
    first.run(1)
    second = trainer.GeoTrainer(geo_net(11), *make_batches(rset), logdir=logdir, precision="bf16", resume=True, quiet=True)
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
    records = second.run(2)                                  # the resumed run goes on with the next epoch
    assert [r["epoch"] for r in records] == [2] and records[0]["iteration"] == 12
    assert len(open(logdir / "metrics.jsonl").read().splitlines()) == 2 and os.path.exists(logdir / "vgn_giga_geo_12.pt")
    assert not os.path.exists(logdir / "vgn_giga_geo_6.pt")
    with pytest.raises(ValueError, match="resume"):
        trainer.GeoTrainer(geo_net(7), *make_batches(rset), logdir=logdir, quiet=True)


def test_geo_command_line_trains_one_epoch(tmp_path, capsys):
    """`python -m giga_amd.train_geo`'s main on a small set in the reference's layout, in this process"""
    from giga_amd import train_geo
    root, raw, out = str(tmp_path / "data"), str(tmp_path / "raw"), tmp_path / "out"
    assert synth.write_training_set(root, raw, n_scenes=2, grasps_per_scene=10, occ_files=(1, 1), n_occ_points=4096, seed=5) == 20
    train_geo.main(["--dataset", root, "--dataset_raw", raw, "--savedir", str(out), "--epochs", "1", "--batch-size", "4", "--val-split",
                    "0.2", "--augment", "--precision", "bf16", "--seed", "2"])
    names = sorted(os.listdir(out))                          # 16 train rows: 4 steps; 4 validation rows: one batch
    assert "vgn_giga_geo_4.pt" in names and "trainer_state.pt" in names
    assert len([n for n in names if n.startswith("best_vgn_giga_geo_val_acc=")]) == 1
    (record,) = [json.loads(line) for line in open(out / "metrics.jsonl")]
    assert record["epoch"] == 1 and record["iteration"] == 4 and list(record["train"]) == list(record["val"]) == list(G.KEYS)
    lines = capsys.readouterr().out.splitlines()
    assert lines[0].startswith("Namespace(") and "net='giga_geo'" in lines[0]
    assert [line.split()[0] for line in lines[1:]] == ["Train", "Val"]
    with pytest.raises(ValueError, match="resume"):          # the directory now holds checkpoints
        train_geo.main(["--dataset", root, "--dataset_raw", raw, "--savedir", str(out), "--epochs", "1", "--batch-size", "4"])
    with pytest.raises(SystemExit):
        train_geo.main(["--dataset", root, "--dataset_raw", raw, "--net", "giga"])


def test_geo_trainer_under_a_process_group(rset, tmp_path):
    """the group's code path in one process (a gloo group of one rank)"""
    import torch.distributed as dist
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    try:
        net = geo_net(7)
        start = net.flatten_parameters()[0].detach().clone()
        train_b, val_b = make_batches(rset)
        none_b = resident.ResidentBatches(rset, 4, shuffle=False, drop_last=True, indices=[1, 2, 3])
        log = StepLog()
        tr = trainer.GeoTrainer(net, train_b, none_b, group=dist.group.WORLD, logdir=tmp_path / "run", on_step=log, quiet=True)
        assert (tr.train_steps, tr.val_steps, tr.rank) == (6, 0, 0)
        assert np.array_equal(bits(start), bits(net.flatten_parameters()[0]))
        (record,) = tr.run(1)
        want, n = log.metrics("train", 0)
        assert n == 6 and record["train"] == want and record["val"] is None and tr.iteration == 6
        tr2 = trainer.GeoTrainer(geo_net(7), train_b, val_b, group=dist.group.WORLD, on_step=log, quiet=True)
        assert (tr2.train_steps, tr2.val_steps) == (6, 1)
        tr2.train_steps = 2                                  # what a rank with a larger share does: it stops with the others
        tr2.train_epoch()
        assert tr2.iteration == 2 and int(tr2.metrics.words()[0]) == 2 and tr2.validate() is not None
    finally:
        dist.destroy_process_group()


def test_geo_batch_loop_adds_no_host_waits(rset):
    """torch's synchronisation warnings inside the batch loop: the GeoTrainer's against a bare loop over the same batches (net,
    geo_loss without metrics, backward, FlatAdam)"""
    net = geo_net(7)
    train_b, _ = make_batches(rset)
    counts = []

    def hook(tr, batch, out, loss_dict):
        counts.append(len(caught))

    tr = trainer.GeoTrainer(net, train_b, precision="bf16", on_step=None)
    opt = FlatAdam(net.flatten_parameters(), lr=2e-4)

    def bare_epoch():
        net.train()
        for x, _, pos_occ, y in train_b:
            opt.zero_grad(set_to_none=True)
            loss, _ = geo_loss(net(x, None, p_tsdf=pos_occ), y[3])
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
    print(f"synchronisation warnings: bare loop {bare}, GeoTrainer's loop {counts[-1]} (whole epoch with the metrics copy {whole})")
    assert counts[-1] <= bare
