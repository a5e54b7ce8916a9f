"""Timing of the query-point gradient (giga_decoder_point_grad, csrc/giga_decoder_pgrad.hip): the qual-head launch at
32 x 2048 and 1 x 64 000 next to the fp32 one-head decoder forward (decoder_f32_kernel) at the same shape, its algorithmic
fraction of the fp32 MFMA peak, and grad_refine's wall time.  Usage: python tools/gpu_point_grad_time.py [out.txt]"""
import sys
import time

import torch

from giga_amd import _capi, synth
from giga_amd.convonet import decoder_point_grad
from giga_amd.networks import get_network
from giga_amd.weights import make_state_dict

PEAK = 157.3e12            # fp32-input MFMA peak of one MI355X
# per point and head: forward recompute (fc_c 5 x 96x32, fc_p, 5 x 2 x 32x32, fc_out) + backward chain (W1^T, W0^T, Wc^T per block,
# Wout^T), 2 FLOP per multiply-add
FLOP_PER_POINT = 2 * 2 * (5 * (96 * 32 + 2 * 32 * 32) + 3 * 32 + 32)
dev = torch.device("cuda:0")
lines = []


def log(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e-3


net = get_network("giga").to(dev)
net.load_state_dict(make_state_dict(7))
net.eval()
blob, bwd = net.packed_blob(dev), net.packed_bwd_blob(dev)
L = _capi.lib()
log(f"FLOP per point and head (forward recompute + backward chain): {FLOP_PER_POINT}")
for B, N in ((32, 2048), (1, 64000)):
    x = torch.from_numpy(synth.tsdf_batch(0, B)).to(dev)
    with torch.no_grad():
        nhwc = net.encoder.encode_nhwc(x, blob=blob, precision="fp32")[0]
    p = torch.from_numpy(synth.query_points(0, B, N, stream=1)).to(dev)
    ones = torch.ones(B, N, device=dev)
    qual = torch.empty(B, N, device=dev)

    def fwd():
        _capi.check(L.giga_decoder_forward(_capi.ptr(nhwc), _capi.ptr(p), _capi.ptr(blob), 1, _capi.ptr(qual), None, None, None,
                                           B, N, 0, 1, _capi.stream_ptr(dev)), "giga_decoder_forward")

    def pgrad():
        decoder_point_grad(nhwc, p, blob, bwd, 1, {"decoder_qual": ones})

    tf, tg = timed(fwd), timed(pgrad)
    frac = FLOP_PER_POINT * B * N / tg / PEAK
    log(f"B={B:2d} N={N:5d}: forward (qual, fp32) {tf * 1e6:7.1f} us | point gradient (qual) {tg * 1e6:7.1f} us = "
        f"{tg / tf:.2f} x forward, {frac:.2f} of the fp32 MFMA peak")

B, N = 1, 64000
x = torch.from_numpy(synth.tsdf_batch(0, B)).to(dev)
pos = torch.from_numpy(synth.query_points(0, B, N, stream=1, half_width=0.45)).to(dev)
for steps in (1, 5):
    for _ in range(3):
        net.grad_refine(x, pos, lr=1e-3, num_step=steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        net.grad_refine(x, pos, lr=1e-3, num_step=steps)
    torch.cuda.synchronize()
    log(f"grad_refine B=1 N=64000 num_step={steps}: {(time.perf_counter() - t0) / 20 * 1e3:.3f} ms (wall, encode + steps + forward)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
