"""Timing of the depth renderer (csrc/giga_render.hip): 1 and 32 scenes x six 480x640 views of a mesh of about 10^4 and about 10^5
triangles (a ground plane and icospheres on the reference's workspace), a whole acquire_tsdf, and render + integrate against the
upload of the images it replaces; each bracketed by HIP events (median of 20 repetitions after warm-up, one process).  Also
recorded: the triangles tested per pixel after the kernel's tile culling (from the workspace counter, see include/giga_hip.h).
Usage: timeout -k 10 600 python tools/gpu_render_time.py [out.txt]   (one GPU step: run it under its own time limit, chained with &&)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_emu as remu  # noqa: E402  (mesh generators)
from giga_amd import perception, render  # noqa: E402

dev = torch.device("cuda:0")
lines = []
SIZE = 0.3
K = render.SIM_INTRINSIC
PIXELS = K[0] * K[1]


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
    log(f"  {name:72s} {med * 1e3:10.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions){extra}")


def scene(subdiv, count):
    """ground plane + `count` icospheres of 20 4^subdiv triangles resting on it"""
    rng = np.random.default_rng(subdiv)
    parts = [remu.plane_mesh(0.05, (-0.5, 0.8, -0.5, 0.8))]
    for _ in range(count):
        r = rng.uniform(0.025, 0.045)
        parts.append(remu.icosphere(np.r_[rng.uniform(0.07, SIZE - 0.07, 2), 0.05 + r], r, subdiv))
    return remu.merge(*parts)


intr = render.sim_intrinsic()
ext = render.acquire_extrinsics(6, None, SIZE)
log(f"depth rendering, six {K[1]}x{K[0]} views per scene on the reference's camera circle; 16x16 pixel tiles")
meshes = {}
for name, (subdiv, count) in (("~1e4 triangles", (4, 2)), ("~1e5 triangles", (5, 5))):
    v, f = scene(subdiv, count)
    meshes[name] = m = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
    for B in (1, 32):
        stats = {}
        depth, _ = render.render_depth_batch([m] * B, intr, [ext] * B, device=dev, stats=stats)
        hit = float((depth < render.SIM_FAR).float().mean())
        per_pixel = stats["tile_pairs"] * 256 / (6 * B * PIXELS)
        row(f"render, {B} scene(s) x 6 views, {len(f)} triangles ({name})", timed(lambda: render.render_depth_batch([m] * B, intr, [ext] * B, device=dev)),
            f"   {per_pixel:.1f} triangles tested per pixel after culling; {hit * 100:.0f} % of the pixels hit")

m = meshes["~1e4 triangles"]
row("acquire_tsdf whole (render, R = 40 and R = 120 volumes, cloud), ~1e4 triangles", timed(lambda: render.acquire_tsdf(m[0], m[1], 6, device=dev)))
depth = render.render_depth(m[0], m[1], intr, ext, device=dev)


def render_and_fuse():
    d = render.render_depth(m[0], m[1], intr, ext, device=dev)
    perception.create_tsdf(SIZE, 40, d, intr, ext, dev)


row("render + integrate at R = 40, ~1e4 triangles (images stay on the device)", timed(render_and_fuse))
host = depth.cpu()
row("upload of six images + integrate at R = 40, pageable host memory", timed(lambda: perception.create_tsdf(SIZE, 40, host, intr, ext, dev)))
row("upload of the six images alone, pageable host memory", timed(lambda: host.to(dev)))
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
