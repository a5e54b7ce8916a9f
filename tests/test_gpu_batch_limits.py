"""The batch limit of include/giga_hip.h (GIGA_MAX_SCENES = 3072 scenes per encoder / training call) and decoder calls whose
outputs pass 2^31 bytes, held to the same scenes run in small chunks and to float64 samples (tests/ref64.py).

Device memory, measured peaks on an MI355X (torch.cuda.max_memory_allocated, printed by every case): the encoder at 3072
scenes 30.4 GB (fp32 workspace 21.8 GB), the lattice decoder 32.4 GB, the generic decoder 48.0 GB, the training step at
3072 scenes x 2048 occupancy points 72-76 GB (encoder workspace 21.8 GB + backward workspace 47.3 GB) and at 1748 scenes
41-44 GB.  The cases run one at a time and free their buffers before the next."""
import gc
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, networks, synth
from giga_amd.training import giga_loss
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402

pytestmark = pytest.mark.gpu

BMAX = _capi.MAX_SCENES
CHUNK = 32
PEAK_LIMIT = 100e9


@pytest.fixture(autouse=True)
def _fresh_memory():
    """Each case starts from an empty allocator and reports its own peak."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated()
    print(f"\nBATCHLIMIT peak device memory {peak / 1e9:.1f} GB")
    gc.collect()
    torch.cuda.empty_cache()
    assert peak <= PEAK_LIMIT


def _net(sd):
    n = networks.get_network("giga")
    n.load_state_dict(sd)
    return n.to(torch.device("cuda:0")).eval()


_X = {}


def _scenes():
    """3072 distinct U[0,1) scenes, the first four adversarial."""
    if "x" not in _X:
        x = synth.tsdf_batch(0, BMAX)
        x[:4] = ref64.adversarial_scenes()
        _X["x"] = torch.from_numpy(x)
    return _X["x"]


def _sample_scenes(B):
    rng = np.random.default_rng(B)
    rand = rng.choice(np.arange(1, B - 4), size=3, replace=False)
    return sorted({0, B - 4, B - 3, B - 2, B - 1, *map(int, rand)})


def _rel(a, b):
    """max |a - b| / max(1, max |b|): the measure of the fuzz test (and of test_batch_256_c3_scene_consistency)."""
    return ((a.float() - b.float()).abs().max() / max(1.0, b.float().abs().max().item())).item()


# ---- encoder at GIGA_MAX_SCENES ---------------------------------------------------------------------------------------
# (label, precision, persistent_unet, bit-identical to chunks, float64 tolerance (range-relative))
# Bit identity holds where the library states batch independence: the f16-class U-Net (persistent == per-layer bit for bit,
# conv16 above 16 scenes, so chunks of 32 and the full batch run the same kernels).  fp32 depends on the batch size at
# rounding level (conv_in's summation order follows the work distribution: INTEGRATION.md section 4), bf16 the same.
ENC_MODES = (("fp32", "fp32", False, False, ref64.TOL["fp32"]), ("fp32-layers", "fp32", "layers", False, ref64.TOL["fp32"]),
             ("fp16x3", "fp16x3", False, True, ref64.TOL["fp16x3"]), ("fp16", "fp16", False, True, 1.5e-2),
             ("bf16", "bf16", False, False, 1.5e-2))


@pytest.mark.parametrize("mode", ENC_MODES, ids=[m[0] for m in ENC_MODES])
def test_encoder_at_max_scenes(sd7, mode):
    label, prec, persist, exact, tol64 = mode
    dev = torch.device("cuda:0")
    net = _net(sd7).set_precision(prec).set_persistent_unet(persist)
    x = _scenes()
    xd = x.to(dev)
    worst = {"chunk": 0.0, "roll": 0.0, "f64": 0.0}
    with torch.no_grad():
        full = net.encode_inputs(xd)
        full = torch.stack([full[k] for k in O.PLANES]).float()         # (3, B, 32, 40, 40)
        for c in range(0, BMAX, CHUNK):
            part = net.encode_inputs(xd[c:c + CHUNK].contiguous())
            part = torch.stack([part[k] for k in O.PLANES]).float()
            if exact:
                assert torch.equal(part, full[:, c:c + CHUNK]), c
            worst["chunk"] = max(worst["chunk"], _rel(full[:, c:c + CHUNK], part))
        # every position again with different content
        rolled = net.encode_inputs(torch.roll(xd, 1537, 0))
        rolled = torch.stack([rolled[k] for k in O.PLANES]).float()
        back = torch.roll(rolled, -1537, 1)
        del rolled
        if exact:
            assert torch.equal(back, full)
        worst["roll"] = _rel(back, full)
        del back
    ks = _sample_scenes(BMAX)
    ref = ref64.encoder(sd7, x[ks])
    for j, k in enumerate(ks):
        e = max(ref64.range_err(full[i, k].cpu(), ref[key][j]) for i, key in enumerate(O.PLANES))
        worst["f64"] = max(worst["f64"], e)
    print(f"\nBATCHLIMIT encoder {label} B={BMAX}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert worst["chunk"] <= 1e-5 and worst["roll"] <= 1e-5, worst
    assert worst["f64"] <= tol64, worst


# ---- decoders past 2^31 bytes -------------------------------------------------------------------------------------------
def _planes_slice(c, sl):
    return {k: c[k][sl] for k in O.PLANES}


@pytest.mark.parametrize("prec", ["fp16x3", "fp16"])
def test_lattice_decoder_at_max_scenes(sd7, prec):
    """3072 scenes x the 64000-point inference lattice: rot alone is 3.1 GB.  Chunks of 32 scenes (one of them straddles
    byte 2^31 of rot) must give the same bits; three scenes against float64."""
    dev = torch.device("cuda:0")
    net = _net(sd7).set_precision(prec)
    x = _scenes()
    lat = torch.from_numpy(synth.inference_lattice()).to(dev)
    with torch.no_grad():
        c = net.encode_inputs(x.to(dev))
        q, r, w = net.decode(lat, c)
        assert r.numel() * 4 >= 2 ** 31
        straddle = (2 ** 31) // (64000 * 16)             # scene whose rot rows cross byte 2^31
        for c0 in (0, straddle - 5, BMAX - CHUNK):
            sl = slice(c0, c0 + CHUNK)
            q1, r1, w1 = net.decode(lat, _planes_slice(c, sl))
            assert torch.equal(q1, q[sl]) and torch.equal(r1, r[sl]) and torch.equal(w1, w[sl]), c0
    ks = [0, straddle, BMAX - 1]
    planes = ref64.encoder(sd7, x[ks])
    _, ref = ref64.heads(sd7, planes, torch.from_numpy(synth.inference_lattice()).expand(len(ks), -1, -1), ref64.HEADS[:3])
    worst = {}
    for j, k in enumerate(ks):
        for name, got, h in (("qual", q, "decoder_qual"), ("rot", r, "decoder_rot"), ("width", w, "decoder_width")):
            g = got[k].cpu()
            worst[name] = max(worst.get(name, 0.0), ref64.range_err(g, ref[h][j]) if prec == "fp16x3" else
                              (g.double() - ref[h][j]).abs().max().item())
    print(f"\nBATCHLIMIT lattice {prec}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    if prec == "fp16x3":
        assert max(worst.values()) <= ref64.TOL["fp16x3"], worst
    else:       # plain f16: the envelope of test_gpu_parity.py::test_inference_lattice_g3_and_predict
        assert worst["qual"] <= 1e-2 and worst["rot"] <= 1.5e-2 and worst["width"] <= 2e-2, worst


def test_generic_decoder_past_2g_rot_elements(sd7):
    """fp32 generic entry point with B * N * 4 >= 2^31 rot elements (8.6 GB): the last chunk of 32 scenes alone gives the same
    bits, and the first and last scene match float64."""
    dev = torch.device("cuda:0")
    net = _net(sd7).set_precision("fp32")
    x = _scenes()
    N = -(-(2 ** 29) // BMAX)
    g = torch.Generator(device=dev).manual_seed(3)
    with torch.no_grad():
        c = net.encode_inputs(x.to(dev))
        p = torch.rand((BMAX, N, 3), device=dev, generator=g) * 1.1 - 0.55
        q, r, w = net.decode(p, c)
        assert r.numel() >= 2 ** 31
        sl = slice(BMAX - CHUNK, BMAX)
        q1, r1, w1 = net.decode(p[sl].contiguous(), _planes_slice(c, sl))
        assert torch.equal(q1, q[sl]) and torch.equal(r1, r[sl]) and torch.equal(w1, w[sl])
    ks = [0, BMAX - 1]
    planes = ref64.encoder(sd7, x[ks])
    _, ref = ref64.heads(sd7, planes, p[ks].cpu(), ref64.HEADS[:3])
    worst = 0.0
    for j, k in enumerate(ks):
        for got, h in ((q, "decoder_qual"), (r, "decoder_rot"), (w, "decoder_width")):
            worst = max(worst, ref64.range_err(got[k].cpu(), ref[h][j]))
    print(f"\nBATCHLIMIT generic fp32 B={BMAX} N={N}: f64 {worst:.2e}")
    assert worst <= ref64.TOL["fp32"]


# ---- training step at 1748 and 3072 scenes --------------------------------------------------------------------------------
def _train_batch(B, M):
    x = _scenes()[:B]
    pos = torch.from_numpy(synth.query_points(0, B, 1, stream=2))
    pos_occ = torch.from_numpy(synth.query_points(0, B, M, stream=3))
    y = tuple(torch.from_numpy(a) for a in synth.train_labels(0, B, M))
    return x, pos, pos_occ, y


def _train_net(sd, prec):
    net = _net(sd).train()
    net.set_train_precision(prec)
    return net


def _grads(net, x, pos, pos_occ, y, weight=1.0):
    dev = torch.device("cuda:0")
    net.zero_grad(set_to_none=True)
    loss, _ = giga_loss(net(x.to(dev), pos.to(dev), p_tsdf=pos_occ.to(dev)), tuple(t.to(dev) for t in y))
    (loss * weight).backward()
    return {n: q.grad.detach().clone() for n, q in net.named_parameters()}


# fp32: summation order only (measured 6.7e-6).  bf16: the chunk's upstream gradients (n_c / B) * (1 / n_c) g and the full
# step's (1 / B) g can differ in their last fp32 bit, and a bf16 operand on a rounding boundary then moves by 2^-8: measured
# 1.95e-4 (B = 1748), 3.6e-5 (B = 3072, where 3072 / 32 is not a power of two either).
TRAIN_TOL = {"fp32": 1e-5, "bf16": 1e-3}


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
@pytest.mark.parametrize("B", [1748, BMAX])
def test_training_step_at_large_batch_equals_chunked_steps(sd7, B, prec):
    """The mean loss is linear over scenes, so one step at B scenes has the scene-weighted average of the gradients of
    steps of <= 32 scenes (each of which test_gpu_training.py::test_gradients_at_batch_32 holds to the oracle), relative to
    each tensor's max |grad| (TRAIN_TOL)."""
    M = 2048
    x, pos, pos_occ, y = _train_batch(B, M)
    net = _train_net(sd7, prec)
    full = _grads(net, x, pos, pos_occ, y)
    del net                                                  # its step buffers: the workspaces of the full batch
    gc.collect()
    torch.cuda.empty_cache()
    net = _train_net(sd7, prec)
    acc = {n: torch.zeros_like(v, dtype=torch.float64) for n, v in full.items()}
    for c in range(0, B, CHUNK):
        sl = slice(c, min(c + CHUNK, B))
        n_c = sl.stop - sl.start
        # the chunk's loss weighted by n_c / B, so that every upstream gradient the kernels round (to bf16 in 'bf16') is the
        # full step's 1/B-scaled value; weighting the chunk's gradient afterwards instead rounds differently (7.5e-3 in bf16)
        part = _grads(net, x[sl], pos[sl], pos_occ[sl], tuple(t[sl] for t in y), n_c / B)
        for n, v in part.items():
            acc[n] += v.double()
    worst = max(((full[n].double() - acc[n]).abs().max() / acc[n].abs().max().clamp_min(1e-30)).item() for n in full)
    print(f"\nBATCHLIMIT train {prec} B={B}: worst |full - chunked| / max|grad| {worst:.2e}")
    bad = {n: ((full[n].double() - acc[n]).abs().max() / acc[n].abs().max()).item() for n in full
           if (full[n].double() - acc[n]).abs().max().item() > TRAIN_TOL[prec] * acc[n].abs().max().item() + 1e-12}
    assert not bad, bad
