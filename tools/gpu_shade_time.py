"""Timing of the colour renderer beside the depth renderer (csrc/giga_render.hip: giga_color_render, giga_depth_render) on the
scenes of tools/gpu_render_time.py: 1 and 32 scenes x six 480x640 views of a ground plane with icospheres of about 10^4 and about
10^5 triangles.  Both entry points get the same packed inputs in one process and are timed interleaved (depth, colour, depth,
...), each call bracketed by HIP events: median of 20 repetitions after warm-up.  A call is the host-side staging copy of the
offsets and cameras plus one kernel.  Also timed: giga_image_downsample on a supersample = 2 render of one scene.
Usage: timeout -k 10 600 python tools/gpu_shade_time.py [out.txt]   (one GPU step: run it under its own time limit, chained with &&)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_emu as remu  # noqa: E402  (mesh generators)
from giga_amd import _capi, ragged, render  # noqa: E402

if not torch.cuda.is_available():
    sys.exit("gpu_shade_time.py measures on a HIP device; none is visible")
dev = torch.device("cuda:0")
lines = []
SIZE = 0.3
K = render.SIM_INTRINSIC
REPS, WARM = 20, 3


def log(s):
    print(s, flush=True)
    lines.append(s)


def scene(subdiv, count):
    """ground plane + `count` icospheres of 20 4^subdiv triangles resting on it (the scenes of tools/gpu_render_time.py)"""
    rng = np.random.default_rng(subdiv)
    parts = [remu.plane_mesh(0.05, (-0.5, 0.8, -0.5, 0.8))]
    for _ in range(count):
        r = rng.uniform(0.025, 0.045)
        parts.append(remu.icosphere(np.r_[rng.uniform(0.07, SIZE - 0.07, 2), 0.05 + r], r, subdiv))
    return remu.merge(*parts)


def interleaved(fns):
    """median, min, max in ms of each of `fns`, called in turn REPS times"""
    for _ in range(WARM):
        for fn in fns:
            fn()
    out = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[i].append(e0.elapsed_time(e1))
    return [(statistics.median(t), min(t), max(t)) for t in out]


W, H = K[0], K[1]
ext6 = render.acquire_extrinsics(6, None, SIZE)
log(f"colour render beside depth render, six {H}x{W} views per scene, same packed inputs, interleaved; HIP events, median of {REPS}")
for name, (subdiv, count) in (("~1e4 triangles", (4, 2)), ("~1e5 triangles", (5, 5))):
    v, f = scene(subdiv, count)
    colors = np.random.default_rng(1).integers(0, 256, size=(len(f), 4), dtype=np.uint8)
    for B in (1, 32):
        n = 6 * B
        vt, vo, ft, fo = ragged.pack_meshes([(v, f)] * B, dev)
        ct, _ = ragged.pack([colors] * B, dev, torch.uint8, cols=4)
        view_offsets = ragged.offsets([6] * B)
        ext = np.ascontiguousarray(np.tile(ext6.reshape(6, 16), (B, 1)))
        cam = np.ascontiguousarray(np.tile(np.array(K[2:], np.float64), (n, 1)))
        lights = np.ascontiguousarray(np.tile(np.array(render.HEADLIGHT, np.float64), (n, 1)))
        bg = np.array([255, 255, 255, 255], np.uint8)
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        depth2 = torch.empty_like(depth)
        rgba = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
        index = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        ws_d = _capi.workspace("giga_depth_render", dev, B, n, int(vo[-1]), int(fo[-1]))
        ws_c = _capi.workspace("giga_color_render", dev, B, n, int(vo[-1]), int(fo[-1]))

        def run_depth():
            _capi.call("giga_depth_render", dev, vt, vo, ft, fo, view_offsets, ext, cam, B, W, H, 0.1, 2.0, 0.0, depth, ws_d, ws_d.numel())

        def run_color(d=depth2, i=index):
            _capi.call("giga_color_render", dev, vt, vo, ft, fo, ct, view_offsets, ext, cam, lights, 0.3, bg, B, W, H, 0.1, 2.0, 0.0,
                       rgba, d, i, ws_c, ws_c.numel())

        def run_color_only():
            run_color(None, None)

        (d_med, d_lo, d_hi), (c_med, c_lo, c_hi), (o_med, o_lo, o_hi) = interleaved([run_depth, run_color, run_color_only])
        assert torch.equal(depth.view(torch.int32), depth2.view(torch.int32))          # what is compared computes the same depth
        hit = float((index >= 0).float().mean())
        log(f"  {B:2d} scene(s) x 6 views, {len(f)} triangles ({name}), {hit * 100:.0f} % of the pixels hit")
        log(f"      giga_depth_render                         {d_med * 1e3:10.1f} us   (min {d_lo * 1e3:.1f}, max {d_hi * 1e3:.1f})")
        log(f"      giga_color_render (colour, depth, index)  {c_med * 1e3:10.1f} us   (min {c_lo * 1e3:.1f}, max {c_hi * 1e3:.1f})   ratio {c_med / d_med:.3f}")
        log(f"      giga_color_render (colour only)           {o_med * 1e3:10.1f} us   (min {o_lo * 1e3:.1f}, max {o_hi * 1e3:.1f})   ratio {o_med / d_med:.3f}")

v, f = scene(4, 2)
colors = np.random.default_rng(1).integers(0, 256, size=(len(f), 4), dtype=np.uint8)
m = (torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev))
ct = torch.from_numpy(colors).to(dev)
intr = render.sim_intrinsic()
fine2 = torch.empty((6, 2 * H, 2 * W, 4), dtype=torch.uint8, device=dev).random_(0, 256)
(one, two, down) = interleaved([lambda: render.render_color(m[0], m[1], ct, intr, ext6, device=dev),
                                lambda: render.render_color(m[0], m[1], ct, intr, ext6, supersample=2, device=dev),
                                lambda: render.downsample(fine2, 2)])
log(f"  render_color whole (Python wrapper), 1 scene x 6 views, ~1e4 triangles: supersample 1 {one[0] * 1e3:.1f} us, supersample 2 "
    f"{two[0] * 1e3:.1f} us; giga_image_downsample of six {2 * H}x{2 * W} images alone {down[0] * 1e3:.1f} us (medians of {REPS})")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
