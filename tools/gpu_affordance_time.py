"""Timing of the affordance kernels (csrc/giga_affordance.hip): one scene at R = 40, a mesh of about 10^5 faces (a ground plane and
five icospheres on the reference's workspace) and about 4000 voxels above th, for each aggregation; giga_affordance_points +
giga_affordance_faces bracketed by HIP events (median of 20 repetitions after warm-up, one process), 'max' both on the cell grid
and in the dense form.  Beside it the numpy restatement of tests/affordance_emu.py on the same host (one run, host
clock): a comparison for the record, not a gate.
Usage: timeout -k 10 600 python tools/gpu_affordance_time.py [out.txt]   (one GPU step: run it under its own time limit, chained with &&)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import affordance_emu as aemu  # noqa: E402
import render_emu as remu  # noqa: E402  (mesh generators)
from giga_amd import visual  # noqa: E402

dev = torch.device("cuda:0")
lines = []
SIZE, R, POINTS = 0.3, 40, 4000


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


rng = np.random.default_rng(0)
parts, centres = [remu.plane_mesh(0.05, (0.0, SIZE, 0.0, SIZE))], []
for _ in range(5):
    r = rng.uniform(0.025, 0.045)
    centres.append(np.r_[rng.uniform(0.07, SIZE - 0.07, 2), 0.05 + r])
    parts.append(remu.icosphere(centres[-1], r, 5))
v, f = remu.merge(*parts)
# quality: blobs about the objects, the POINTS strongest voxels above th
g = np.stack(np.meshgrid(*(np.linspace(0, SIZE, R),) * 3, indexing="ij"), -1)
field = sum(np.exp(-((g - c) ** 2).sum(-1) / 0.002) for c in centres) + 0.05 * rng.random((R, R, R))
cut = np.sort(field.reshape(-1))[-POINTS]
qual = np.where(field >= cut, 0.55 + 0.4 * (field - cut) / (field.max() - cut), 0.2).astype(np.float32)
rot = rng.standard_normal((R, R, R, 4)).astype(np.float32)
rot /= np.linalg.norm(rot, axis=-1, keepdims=True)
P = int((qual > np.float32(0.5)).sum())
log(f"affordance of one scene: R = {R}, {len(f)} faces, {P} points above th = 0.5, rad = 0.02, temp = 150")
mesh = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
q_d, r_d = torch.from_numpy(qual).to(dev), torch.from_numpy(rot).to(dev)
for aggregation, dense in (("max", False), ("max", True), ("softmax", False), ("mean", False)):
    run = visual._Affordance(q_d, r_d, [mesh], aggregation=aggregation, dense=dense)
    med, lo, hi = timed(run.launch)
    aff, rgba = run.finish()[0]
    t0 = time.perf_counter()
    want = aemu.affordance(qual, rot, v, f, aggregation=aggregation) if not dense else None
    host = time.perf_counter() - t0
    form = "dense" if dense or aggregation != "max" else "cell grid"
    extra = ""
    if want is not None:
        err = np.nanmax(np.abs(aff.cpu().numpy() - want[1]))
        same = np.array_equal(rgba.cpu().numpy(), want[2])
        extra = f"   numpy restatement on the host {host:.1f} s; max |device - restatement| {err:.1e}, colours {'equal' if same else 'DIFFER'}"
    log(f"  {aggregation:8s} ({form:9s}) points + faces {med * 1e3:10.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions){extra}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
