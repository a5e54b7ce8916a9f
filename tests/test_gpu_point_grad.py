"""GPU tests of the query-point gradients (giga_decoder_point_grad, csrc/giga_decoder_pgrad.hip): the ABI against float64
autograd of the oracle decoder on the GPU's own planes, the autograd paths of the model API, grad_refine and
Generator3D.estimate_normals against the restatement of tests/pgrad_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import networks, synth, weights
from giga_amd.convonet import decoder_point_grad
from giga_amd.generation import Generator3D
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgrad_ref  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = pgrad_ref.HEADS
_NETS = {}


def _net(seed):
    if seed not in _NETS:
        net = networks.get_network("giga")
        net.load_state_dict(weights.make_state_dict(seed))
        _NETS[seed] = net.to(DEV).eval()
    return _NETS[seed]


def _points(first, B, N):
    """Mostly inside the cube; every 64th point (offset 1) outside it (clamped: only fc_p's term is left), offset 2 on the
    40^3 inference lattice; every 128th (offset 3) with x at pixel 0 of its planes."""
    p = synth.query_points(first, B, N, stream=7, half_width=0.5).copy()
    out = synth.query_points(first, B, N, stream=8, half_width=0.8)
    lat = O.inference_lattice(40)[0].numpy()
    idx = np.arange(N)
    p[:, idx % 64 == 1] = out[:, idx % 64 == 1]
    sel = np.nonzero(idx % 64 == 2)[0]
    p[:, sel] = lat[(sel * 7919 + first) % lat.shape[0]]
    p[:, idx % 128 == 3, 0] = np.float32(-0.5 * 1.00001)
    return torch.from_numpy(p)


def _excluded(pre, p, B):
    """Points whose float64 oracle has a ReLU input within 1e-5 (relative to that layer's max) of zero, or a sample
    coordinate within 1e-4 px of a cell edge: there the one-sided derivatives of fp32 and float64 may differ."""
    bad = torch.zeros(p.shape[:2], dtype=torch.bool)
    for t in pre:
        m = t.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)
        bad |= ((t.abs() / m) < 1e-5).any(dim=-1)
    v = p.double() / (1 + 10e-6) + 0.5                   # (a clamped coordinate has zero derivative in both)
    fx = v * 39
    bad |= (((fx - fx.round()).abs() < 1e-4) & (v > -1e-6) & (v < 1 + 1e-6)).any(dim=-1)
    return bad


CASES = [(seed, B, N, [1, 2, 4, 7, 8][(i + j + seed) % 5]) for seed in (7, 11) for i, B in enumerate((1, 3, 32))
         for j, N in enumerate((1, 31, 33, 2048))] + [(7, 3, 33, m) for m in (1, 2, 4, 7, 8, 15)]


@pytest.mark.parametrize("seed, B, N, mask", CASES)
def test_abi_matches_oracle_autograd(seed, B, N, mask):
    net = _net(seed)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    x = torch.from_numpy(synth.tsdf_batch(seed, B))
    with torch.no_grad():
        c = net.encode_inputs(x.to(DEV))                      # final planes, fp32
    planes = {k: c[k].cpu() for k in O.PLANES}
    p = _points(seed + B, B, N)
    gen = torch.Generator().manual_seed(seed * 100 + B * 10 + N)
    douts = {}
    for i, h in enumerate(HEADS):
        if mask >> i & 1:
            douts[h] = torch.randn((B, N, 4) if i == 1 else (B, N), generator=gen)
    blob, bwd = net.packed_blob(DEV), net.packed_bwd_blob(DEV)
    dp, outs = decoder_point_grad(c.nhwc, p.to(DEV), blob, bwd, mask, {h: d.to(DEV) for h, d in douts.items()},
                                  want_outputs=True)
    torch.cuda.synchronize()
    pre = []
    ref = pgrad_ref.point_grad(sd, planes, p, douts, pre)
    bad = _excluded(pre, p, B)
    if B * N >= 1024:           # the ReLU criterion alone takes ~1.2 % of the points per head (measured, both seeds); the
        # points placed at pixel 0 sit on a cell edge by construction and are not counted
        placed = torch.from_numpy(np.arange(N) % 128 == 3).expand(B, N)
        assert (bad & ~placed).float().mean().item() < 0.02 * len(douts), (bad & ~placed).float().mean().item()
    got = dp.cpu().double()
    # the rot head's F.normalize backward amplifies fp32 rounding (d rot / d z ~ 1/|z|): where torch's own fp32 autograd misses
    # 1e-4 of the scene's max, the kernel may miss by as much as twice torch's fp32 error
    ref32 = pgrad_ref.point_grad(sd, planes, p, douts, dtype=torch.float32).double() if mask & 2 else None
    for b in range(B):
        keep = ~bad[b]
        scale = ref[b].abs().max().item()
        err = (got[b][keep] - ref[b][keep]).abs().max().item() if keep.any() else 0.0
        tol = 1e-4 * scale + 1e-12
        if ref32 is not None and keep.any():
            tol = max(tol, 2 * (ref32[b][keep] - ref[b][keep]).abs().max().item())
        assert err <= tol, (b, err, scale, tol)
    # the by-product outputs are decoder_f32_kernel's values bit for bit (N = 1 takes the forward's few-point kernel)
    with torch.no_grad():
        fwd = net.decode(p.to(DEV), c) if mask & 7 else ()
        occ = net.decode_occ(p.to(DEV), c).logits if mask & 8 else None
    for i, h in enumerate(HEADS[:3]):
        if mask >> i & 1:
            assert torch.equal(outs[h], fwd[i]) if N > 1 else torch.allclose(outs[h], fwd[i], atol=1e-5), h
    if mask & 8:
        assert torch.equal(outs["decoder_tsdf"], occ) if N > 1 else torch.allclose(outs["decoder_tsdf"], occ, atol=1e-5)


def test_frozen_autograd_of_forward_and_decode_occ_equals_abi():
    net = _net(7)
    net.requires_grad_(False)
    try:
        B, N = 3, 40
        x = torch.from_numpy(synth.tsdf_batch(2, B)).to(DEV)
        p = _points(4, B, N).to(DEV)
        gen = torch.Generator().manual_seed(3)
        dq, dr, dw, dt = (torch.randn(s, generator=gen).to(DEV) for s in ((B, N), (B, N, 4), (B, N), (B, N)))
        with torch.no_grad():
            ref_vals = net(x, p, p_tsdf=p)
        pg = p.clone().requires_grad_(True)
        pt = p.clone().requires_grad_(True)
        out = net(x, pg, p_tsdf=pt)
        for a, b in zip(out, ref_vals):                      # values are the inference path's, bit for bit
            assert torch.equal(a.detach(), b)
        assert all(t.grad_fn is not None for t in out)
        g, gt = torch.autograd.grad((out[0] * dq).sum() + (out[1] * dr).sum() + (out[2] * dw).sum() + (out[3] * dt).sum(),
                                    (pg, pt))
        blob, bwd = net.packed_blob(DEV), net.packed_bwd_blob(DEV)
        with torch.no_grad():
            nhwc = net.encoder.encode_nhwc(x, blob=blob, precision="fp32")[0]
        ref = decoder_point_grad(nhwc, p, blob, bwd, 7, dict(zip(HEADS[:3], (dq, dr, dw))))
        ref_t = decoder_point_grad(nhwc, p, blob, bwd, 8, {"decoder_tsdf": dt})
        assert torch.allclose(g, ref, rtol=1e-5, atol=1e-6 * ref.abs().max().item())
        assert torch.allclose(gt, ref_t, rtol=1e-5, atol=1e-6 * ref_t.abs().max().item())
        # decode_occ(p, c).logits and decode(p, c) on the encoder's planes
        with torch.no_grad():
            c = net.encode_inputs(x)
        pg = p.clone().requires_grad_(True)
        logits = net.decode_occ(pg, c).logits
        (g,) = torch.autograd.grad((logits * dt).sum(), pg)
        assert torch.equal(g, decoder_point_grad(c.nhwc, p, blob, bwd, 8, {"decoder_tsdf": dt}))
        pg = p.clone().requires_grad_(True)
        q, r, w = net.decode(pg, c)
        (g,) = torch.autograd.grad((q * dq).sum() + (r * dr).sum() + (w * dw).sum(), pg)
        assert torch.equal(g, decoder_point_grad(c.nhwc, p, blob, bwd, 7, dict(zip(HEADS[:3], (dq, dr, dw)))))
        # infer_geo
        pg = p.clone().requires_grad_(True)
        (g,) = torch.autograd.grad((net.infer_geo(x, pg) * dt).sum(), pg)
        assert torch.allclose(g, ref_t, rtol=1e-5, atol=1e-6 * ref_t.abs().max().item())
    finally:
        net.requires_grad_(True)


def test_geometry_model_point_autograd():
    sd = weights.make_state_dict(11, heads=("decoder_tsdf",))
    geo = networks.get_network("giga_geo")
    geo.load_state_dict(sd)
    geo = geo.to(DEV).eval().requires_grad_(False)
    B, N = 2, 50
    x = torch.from_numpy(synth.tsdf_batch(9, B))
    p = torch.from_numpy(synth.query_points(9, B, N, stream=7, half_width=0.45))      # (away from the clamp boundary)
    pg = p.clone().to(DEV).requires_grad_(True)
    (g,) = torch.autograd.grad(geo(x.to(DEV), None, pg).sum(), pg)
    ref = pgrad_ref.point_grad(sd, O.encoder_forward(sd, x), p, {"decoder_tsdf": torch.ones(B, N)})
    assert (g.cpu().double() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()
    with torch.no_grad():
        c = geo.encode_inputs(x.to(DEV))
    pg = p.clone().to(DEV).requires_grad_(True)
    (g2,) = torch.autograd.grad(geo.decode_occ(pg, c).logits.sum(), pg)
    assert torch.allclose(g, g2, rtol=1e-4, atol=1e-5 * ref.abs().max().item())


def _train_run(net, x, pos, pos_occ, gouts, p_grad):
    for q in net.parameters():
        q.grad = None
    pg = pos.clone().requires_grad_(p_grad)
    pt = pos_occ.clone().requires_grad_(p_grad)
    out = net(x, pg, p_tsdf=pt)
    sum((o * g).sum() for o, g in zip(out, gouts)).backward()
    return [q.grad.clone() for q in net.parameters()], pg.grad, pt.grad


def test_training_path_point_gradients_leave_parameter_gradients(sd7):
    """The training autograd function with p / p_tsdf requiring grad: dp and dp_tsdf against float64, and the parameter
    gradients are what they are without the point gradients.  62 of the 164 parameter gradients are reduced with fp32
    atomics (the decoders' plane gradient and weight gradients) and change from run to run, some among only a handful of
    values, so two runs that agree bit for bit do not make a tensor deterministic.  K_BASE runs without point gradients
    decide it: a tensor equal in all of them must come out bit for bit the same in every run with point gradients; any other
    tensor must stay within 4x the run-to-run spread."""
    K_BASE, K_WITH = 32, 4
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    net = net.to(DEV).train()
    B, N, M = 2, 5, 96
    x = torch.from_numpy(synth.tsdf_batch(11, B))
    pos = torch.from_numpy(synth.query_points(12, B, N, stream=7, half_width=0.45))
    pos_occ = torch.from_numpy(synth.query_points(13, B, M, stream=7, half_width=0.45))
    gen = torch.Generator().manual_seed(5)
    gouts = [torch.randn(s, generator=gen) for s in ((B, N), (B, N, 4), (B, N), (B, M))]
    xd, pd, pod, gd = x.to(DEV), pos.to(DEV), pos_occ.to(DEV), [g.to(DEV) for g in gouts]
    base = []
    for _ in range(K_BASE):
        grads, none_p, none_t = _train_run(net, xd, pd, pod, gd, False)
        assert none_p is None and none_t is None
        base.append(grads)
    with_p = [_train_run(net, xd, pd, pod, gd, True) for _ in range(K_WITH)]
    names = [n for n, _ in net.named_parameters()]
    n_det = 0
    for i, name in enumerate(names):
        a = base[0][i]
        runs = [r[i] for r in base]
        if all(torch.equal(a, r) for r in runs[1:]):        # deterministic tensor: bitwise
            n_det += 1
            for c, _, _ in with_p:
                assert torch.equal(a, c[i]), name
        else:                                              # fp32 atomics: within the run-to-run spread
            spread = max((a - r).abs().max().item() for r in runs[1:])
            for c, _, _ in with_p:
                assert (a - c[i]).abs().max().item() <= 4 * spread + 1e-7 * a.abs().max().item(), name
    assert n_det > 0
    ref = pgrad_ref.point_grad(sd7, O.encoder_forward(sd7, x), pos, dict(zip(HEADS[:3], gouts[:3])))
    ref_t = pgrad_ref.point_grad(sd7, O.encoder_forward(sd7, x), pos_occ, {"decoder_tsdf": gouts[3]})
    for _, dp, dpt in with_p:
        assert (dp.cpu().double() - ref).abs().max().item() < 1e-3 * ref.abs().max().item()
        assert (dpt.cpu().double() - ref_t).abs().max().item() < 1e-3 * ref_t.abs().max().item()


def test_bf16_decoder_training_with_point_grad_raises(sd7):
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    net = net.to(DEV).train().set_train_precision("bf16")
    x = torch.from_numpy(synth.tsdf_batch(1, 1)).to(DEV)
    p = torch.zeros(1, 2, 3, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError):
        net(x, p, p_tsdf=torch.zeros(1, 8, 3, device=DEV))


@pytest.mark.parametrize("lr, num_step", [(1e-6, 1), (1e-3, 3)])
def test_grad_refine_matches_restatement(sd7, lr, num_step):
    net = networks.get_network("giga")
    net.load_state_dict(sd7)
    net = net.to(DEV).train()
    B, N = 2, 48
    x = torch.from_numpy(synth.tsdf_batch(20, B, realistic=True))
    pos = torch.from_numpy(synth.query_points(20, B, N, stream=4, half_width=0.45))
    q, p, r, w = net.grad_refine(x.to(DEV), pos.to(DEV), lr=lr, num_step=num_step)
    qr, pr, rr, wr = pgrad_ref.grad_refine(sd7, x, pos, lr=lr, num_step=num_step)
    assert not net.training
    assert all(t.grad is None for t in net.parameters())
    assert (p.cpu().double() - pr).abs().max().item() < 1e-6
    if lr > 1e-5:
        assert (p.cpu() - pos).abs().max().item() > 1e-5                # the points did move
    for a, b in ((q, qr), (r, rr), (w, wr)):
        assert (a.cpu() - b).abs().max().item() < 1e-4


def test_estimate_normals_matches_restatement(sd7):
    net = _net(7)
    gen = Generator3D(net, points_batch_size=100, device=DEV)
    x = torch.from_numpy(synth.tsdf_batch(21, 1, realistic=True))
    c = gen.encode(x)
    v = synth.query_points(21, 1, 333, stream=6, half_width=0.45)[0]
    n_host = gen.estimate_normals(v, c)                                   # host input: chunks of 100
    n_dev = gen.estimate_normals(torch.from_numpy(v).to(DEV), c)          # device input: one launch
    assert n_host.shape == (333, 3) and isinstance(n_host, np.ndarray)
    assert np.array_equal(n_host, n_dev)
    planes = {k: c[k].cpu() for k in O.PLANES}
    ref = pgrad_ref.estimate_normals({k: t.detach().cpu() for k, t in net.state_dict().items()}, planes, v)
    g = pgrad_ref.point_grad({k: t.detach().cpu() for k, t in net.state_dict().items()}, planes,
                             torch.from_numpy(v)[None], {"decoder_tsdf": torch.ones(1, 333)})[0]
    assert np.abs(np.linalg.norm(n_host, axis=-1) - 1).max() < 1e-5
    big = g.norm(dim=-1).numpy() > 1e-3 * g.norm(dim=-1).max().item()
    cos = (n_host.astype(np.float64) * ref).sum(-1)
    assert cos[big].min() > 0.9999, cos[big].min()
