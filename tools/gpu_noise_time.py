"""Timing of the depth noise (csrc/giga_noise.hip): each model on 32 and on 192 images (32 scenes x 6 views) of 480 x 640, and the
giga_tsdf_integrate launch that consumes the same images (40^3 volumes; 6 views per volume, and one), so that the cost of the noise can be
read against the step it precedes; each bracketed by HIP events (median of 20 repetitions after warm-up, one process).  The rate is
against the algorithmic traffic of 8 bytes per pixel (one float32 read, one written).
Usage: python tools/gpu_noise_time.py [out.txt]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import tsdf_emu as emu  # noqa: E402
from giga_amd import noise, perception  # noqa: E402

dev = torch.device("cuda:0")
lines = []
H, W, VIEWS, SIZE = 480, 640, 6, 0.3


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


log(f"depth noise on {H} x {W} float32 images; HIP events around the Python call, median of 20 repetitions (min, max)")
ext = emu.six_views(SIZE, VIEWS, VIEWS)
base = torch.from_numpy(emu.render_views(emu.make_scene(11), ext, emu.SIM_INTRINSIC)).to(dev)          # (6, 480, 640)
intr = perception.CameraIntrinsic(*emu.SIM_INTRINSIC)
for scenes in (32 // VIEWS + 1, 32):
    n = 32 if scenes != 32 else scenes * VIEWS
    depth = base.repeat(scenes, 1, 1)[:n].contiguous()
    log(f"{n} images ({n * H * W * 4 / 1e6:.0f} MB in, as much out)")
    for kind in ("dex", "trans", "norm"):
        nz = noise.DepthNoise(kind, seed=1)
        med, lo, hi = timed(lambda: nz.apply(depth))
        log(f"  {kind:5s} {med * 1e3:9.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})   {n * H * W * 8 / (med * 1e-3) / 1e9:7.0f} GB/s of 8 B/pixel")
    for per in (VIEWS, 1):
        if n % per:
            continue
        B = n // per
        tsdf = torch.zeros((B, 40, 40, 40), device=dev)
        weight, grid = torch.zeros_like(tsdf), torch.zeros_like(tsdf)
        offs = np.arange(B + 1) * per
        cams = [ext[k % VIEWS] for k in range(n)]

        def fuse():
            tsdf.zero_(), weight.zero_()
            perception.integrate_batch(tsdf, weight, depth, offs, intr, cams, SIZE, grid)

        def clear():
            tsdf.zero_(), weight.zero_()

        med, lo, hi = timed(fuse)
        c = timed(clear)[0]
        log(f"  giga_tsdf_integrate of the same images into {B} volumes of 40^3, {per} per volume (with its two clears, {c * 1e3:.1f} us, and the upload of "
            f"{n} cameras): {med * 1e3:9.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
