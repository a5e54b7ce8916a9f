"""Timing of the mesh evaluation (csrc/giga_eval.hip): nearest neighbours at 100 000 x 100 000, surface sampling and containment of
100 000 points on the 129^3 mesh of tools/gpu_mesh_time.py, and a whole eval_mesh call; each bracketed by HIP events (median of 20
repetitions after warm-up, one process), with the achieved pair rate of the two brute-force kernels.
Usage: python tools/gpu_eval_time.py [out.txt]"""
import statistics
import sys
import time

import numpy as np
import torch

from giga_amd import eval as E
from giga_amd import synth
from giga_amd.generation import Generator3D
from giga_amd.networks import get_network
from giga_amd.weights import make_state_dict

dev = torch.device("cuda:0")
lines = []
N = 100000
VALU_PEAK = 157.3e12 / 2          # fp32 vector lanes x clock: one non-fused operation per lane and cycle


def log(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out), min(out), max(out)


def row(name, t, extra=""):
    med, lo, hi = t
    log(f"  {name:58s} {med * 1e3:10.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions){extra}")


net = get_network("giga").to(dev)
net.load_state_dict(make_state_dict(7))
net.eval()
gen = Generator3D(net, device=dev, threshold=0.6)
mesh = gen.generate_mesh({"inputs": torch.from_numpy(synth.tsdf_batch(70, 1)).to(dev)}, return_stats=False)
v, f = torch.from_numpy(mesh.vertices).to(dev), torch.from_numpy(mesh.faces).to(dev).to(torch.int32)
nf = len(f)
log(f"mesh evaluation, scene 70, weight seed 7, threshold 0.6, 129^3 samples: {len(v)} vertices, {nf} triangles; {N} points per cloud")
pred, _, normals = E.sample_surface((v, f), N, seed=0)
tgt = pred * 1.02 + 0.003
n_tgt = normals.clone()
rng = np.random.default_rng(0)
pts = torch.from_numpy(rng.random((N, 3)) - 0.5).to(dev)
occ_tgt = (pts.norm(dim=1) < 0.3).cpu().numpy()

t = timed(lambda: E.nn_query_batch([pred], [tgt]))
row("nearest neighbour, 100 000 x 100 000, one direction", t, f"   {N * N / (t[0] * 1e-3):.3g} pairs/s")
t2 = timed(lambda: (E.nn_query_batch([pred], [tgt]), E.nn_query_batch([tgt], [pred])))
row("nearest neighbour, both directions", t2, f"   {2 * N * N / (t2[0] * 1e-3):.3g} pairs/s")
log(f"    a pair costs 11 fp32 vector operations (3 differences, 3 products, 2 sums, compare, 2 selects), none fused: the VALU peak of "
    f"{VALU_PEAK:.3g} lane-operations/s allows {VALU_PEAK / 11:.3g} pairs/s; achieved {N * N / (t[0] * 1e-3) / (VALU_PEAK / 11) * 100:.0f} % of that")
row("surface sampling, 100 000 points (areas, scan, draw)", timed(lambda: E.sample_surface((v, f), N, seed=0)))
t = timed(lambda: E.check_mesh_contains((v, f), pts))
inside = int(E.check_mesh_contains((v, f), pts).sum())
row(f"containment, 100 000 points, hash_resolution 512 ({inside} inside)", t, f"   {N * nf / (t[0] * 1e-3):.3g} point-triangle cell tests/s")
ev = E.MeshEvaluator(n_points=N)
row("whole eval_mesh (sample, 2 x nn, reductions, containment, iou)", timed(lambda: ev.eval_mesh((v, f), tgt, n_tgt, pts, occ_tgt), reps=20, warm=2))
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(5):
    out = ev.eval_mesh((v, f), tgt, n_tgt, pts, occ_tgt)
log(f"  whole eval_mesh call, wall: {(time.perf_counter() - t0) / 5 * 1e3:.2f} ms   chamfer-L1 {out['chamfer-L1']:.6f}  f-score {out['f-score']:.4f}  iou {float(out['iou']):.4f}")
log("  for orientation: the reference's CPU time when tests/golden/g17_eval.npz was made (fixture A, 4 168 faces): KD-tree build + query, "
    "20 000 x 20 000 in both directions 0.030 s; check_mesh_contains of 20 000 points 0.034 s")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
