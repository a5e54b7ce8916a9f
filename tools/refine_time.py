"""Timing of the mesh refinement (giga_amd.refine, csrc/giga_refine.hip, giga_decoder_point_hess): the four launches of a step
on the default 129^3 marching-cubes mesh of a synthetic scene, a whole step and Generator3D's wall time with and without
refinement, and the point-hess launch next to giga_decoder_point_grad (occupancy head) at 32 x 2048 in the same run.
Usage: python tools/refine_time.py [out.txt]   (profiles/refine/refine_time.txt)"""
import sys
import time

import torch

from giga_amd import _capi, synth
from giga_amd.generation import Generator3D
from giga_amd.networks import get_network
from giga_amd.refine import MeshRefiner
from giga_amd.weights import make_state_dict

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
P, S = _capi.ptr, _capi.stream_ptr

# ---- point-hess against the point gradient, occupancy head, preallocated outputs, alternating -------------------------------
B, N = 32, 2048
x = torch.from_numpy(synth.tsdf_batch(0, B)).to(dev)
with torch.no_grad():
    nhwc = net.encoder.encode_nhwc(x, blob=blob, precision="fp32")[0]
p = torch.from_numpy(synth.query_points(0, B, N, stream=1)).to(dev)
ones, logit = torch.ones(B, N, device=dev), torch.empty(B, N, device=dev)
dp, hess = torch.empty(B, N, 3, device=dev), torch.empty(B, N, 3, device=dev)


def pgrad():
    _capi.check(L.giga_decoder_point_grad(P(nhwc), P(p), P(blob), P(bwd), 8, None, None, None, P(ones), P(dp), None, None, None,
                                          P(logit), B, N, 0, S(dev)), "giga_decoder_point_grad")


def phess():
    _capi.check(L.giga_decoder_point_hess(P(nhwc), P(p), P(blob), P(bwd), P(logit), P(dp), P(hess), B, N, S(dev)),
                "giga_decoder_point_hess")


for rnd in range(3):
    tg, th = timed(pgrad), timed(phess)
    log(f"B={B} N={N} round {rnd}: point gradient (occupancy head, with logits) {tg * 1e6:6.1f} us | point-hess {th * 1e6:6.1f} us "
        f"= {th / tg:.3f} x")

# ---- one refinement step on the default mesh --------------------------------------------------------------------------------
x1 = torch.from_numpy(synth.tsdf_batch(70, 1)).to(dev)
gen = Generator3D(net, device=dev)                               # resolution0 16, 3 upsampling steps: 129^3 samples
c = gen.encode(x1)
mesh = gen.generate_from_latent(c)
r = MeshRefiner(net, c, mesh.vertices, mesh.faces, threshold=gen.threshold, seed=0)
V, F = r.vertices.shape[0], r.faces.shape[0]
log(f"mesh of synthetic scene 70 at 129^3: {V} vertices, {F} faces")
r.step()
fp = r.face_points[None].contiguous()
lg, dq, hs = torch.empty(1, F, device=dev), torch.empty(1, F, 3, device=dev), torch.empty(1, F, 3, device=dev)
launches = (
    ("giga_refine_face_points (drawn weights)", lambda: L.giga_refine_face_points(
        P(r.vertices), P(r.faces), None, P(r.eps), P(r.face_points), V, F, 0, 1, S(dev))),
    ("giga_decoder_point_hess (1 x F)", lambda: L.giga_decoder_point_hess(
        P(r.nhwc), P(fp), P(blob), P(bwd), P(lg), P(dq), P(hs), 1, F, S(dev))),
    ("giga_refine_face_grad", lambda: L.giga_refine_face_grad(
        P(r.vertices), P(r.faces), P(r.eps), P(lg), P(dq), P(hs), 0.5, P(r.face_loss), P(r.face_grad), V, F, S(dev))),
    ("giga_refine_vertex_step", lambda: L.giga_refine_vertex_step(
        P(r.face_grad), P(r.corner_order), P(r.vertex_offsets), P(r.vertices), P(r.square_avg), P(r.grad), V, F, S(dev))),
)
total = 0.0
with torch.cuda.device(dev):
    for name, fn in launches:
        t = timed(fn)
        total += t
        log(f"  {name:42s} {t * 1e6:7.1f} us")
log(f"  sum of the four launches                   {total * 1e6:7.1f} us")
log(f"  MeshRefiner.step() (with its allocations)  {timed(r.step) * 1e6:7.1f} us")
t0 = time.perf_counter()
MeshRefiner(net, c, mesh.vertices, mesh.faces)
torch.cuda.synchronize()
log(f"  MeshRefiner(...) from host arrays (upload, index check, stable sort): {(time.perf_counter() - t0) * 1e3:.2f} ms")

for steps in (0, 30):
    g = Generator3D(net, device=dev, refinement_step=steps)
    for _ in range(2):
        g.generate_mesh({"inputs": x1})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        g.generate_mesh({"inputs": x1})
    torch.cuda.synchronize()
    log(f"generate_mesh, 129^3, refinement_step={steps:2d}: {(time.perf_counter() - t0) / 5 * 1e3:.2f} ms (wall)")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
