"""Timing of the depth fusion (csrc/giga_tsdf.hip): integrate + export for 1 and 32 scenes x six 480x640 views at R = 40 and for one
scene at R = 120, cloud count and emit, the upload of the images on its own, and a whole plan_from_depth call; each bracketed by HIP
events (median of 20 repetitions after warm-up, one process) and put against the bytes it must move: the 128-byte lines of the
depth images that some voxel reads, plus the state and grid read and written (20 bytes per voxel).
Usage: timeout -k 10 600 python tools/gpu_tsdf_time.py [out.txt]   (one GPU step: run it under its own time limit, chained with &&)"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tsdf_emu as emu  # noqa: E402  (analytic depth renderer and the reference's camera circle)
from giga_amd import _capi, perception  # noqa: E402
from giga_amd.detection import VGNImplicit  # noqa: E402
from giga_amd.networks import get_network  # noqa: E402
from giga_amd.weights import make_state_dict  # noqa: E402

dev = torch.device("cuda:0")
lines = []
SIZE = 0.3
K = emu.SIM_INTRINSIC
HBM_PEAK = 8.0e12          # bytes/s, the MI355X's HBM3E rate


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


def row(name, t, nbytes=None):
    med, lo, hi = t
    extra = ""
    if nbytes:
        extra = f"   {nbytes / 1e6:.2f} MB to move -> {nbytes / (med * 1e-3) / 1e9:.0f} GB/s ({nbytes / (med * 1e-3) / HBM_PEAK * 100:.1f} % of HBM peak)"
    log(f"  {name:64s} {med * 1e3:10.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions){extra}")


def depth_lines_touched(ext, R):
    """128-byte lines (32 pixels of a row) of the views' images that at least one voxel reads; float64 projection of every voxel
    centre.  Depends on the cameras only, not on the scene."""
    W, H, fx, fy, cx, cy = K
    c = (np.arange(R) + 0.5) * (SIZE / R)
    P = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(-1, 3)
    n = 0
    for E in ext:
        pc = P @ E[:3, :3].T + E[:3, 3]
        ok = pc[:, 2] > 0
        u = pc[ok, 0] * fx / pc[ok, 2] + cx + 0.5
        v = pc[ok, 1] * fy / pc[ok, 2] + cy + 0.5
        inside = (u >= 0.0001) & (u < W - 0.0001) & (v >= 0.0001) & (v < H - 0.0001)
        n += len(np.unique(v[inside].astype(np.int64) * ((W + 31) // 32) + u[inside].astype(np.int64) // 32))
    return n


ext = emu.six_views(SIZE)
intr = perception.CameraIntrinsic(*K)
depth1 = emu.render_views(emu.make_scene(70), ext, K)
image_bytes = depth1.nbytes
log(f"depth fusion, six {K[1]}x{K[0]} views per scene on the reference's camera circle, volume {SIZE} m; {image_bytes / 1e6:.2f} MB of images per scene")


def fusion_rows(B, R):
    depth = torch.from_numpy(np.concatenate([depth1] * B)).to(dev)
    offs = np.ascontiguousarray(np.arange(B + 1) * 6, np.int32)
    ext16 = np.ascontiguousarray(np.tile(ext.reshape(6, 16), (B, 1)))
    cam4 = np.ascontiguousarray(np.tile(np.array(K[2:], np.float64), (6 * B, 1)))
    tsdf = torch.zeros((B, R, R, R), device=dev)
    weight, grid = torch.zeros_like(tsdf), torch.zeros_like(tsdf)
    L = _capi.lib()
    ws = torch.empty(L.giga_tsdf_integrate_workspace_bytes(B, 6 * B), dtype=torch.uint8, device=dev)
    stream = _capi.stream_ptr(dev)

    def run():                                   # the C ABI call itself (camera arrays prepared once): two memsets, two small H2D copies, one kernel
        tsdf.zero_()
        weight.zero_()
        _capi.check(L.giga_tsdf_integrate(_capi.ptr(depth), offs.ctypes.data, ext16.ctypes.data, cam4.ctypes.data, B, K[0], K[1], SIZE, R,
                                          4.0 * (SIZE / R), 1.0, 2.0, _capi.ptr(tsdf), _capi.ptr(weight), _capi.ptr(grid), _capi.ptr(ws),
                                          ws.numel(), stream), "giga_tsdf_integrate")
    lines128 = depth_lines_touched(ext, R)
    nbytes = B * (lines128 * 128 + 20 * R ** 3)
    row(f"integrate + export, {B} scene(s) x 6 views, R = {R} (memsets of a new volume and camera upload included)", timed(run), nbytes)
    log(f"      per scene: {lines128} depth lines of 128 B touched ({lines128 * 128 / 1e6:.2f} MB of the {image_bytes / 1e6:.2f} MB), "
        f"state + grid {20 * R ** 3 / 1e6:.2f} MB; {6 * R ** 3 * B} voxel-views")
    run()
    return tsdf, weight


tsdf1, weight1 = fusion_rows(1, 40)
tsdf32, weight32 = fusion_rows(32, 40)
tsdf120, weight120 = fusion_rows(1, 120)
for name, (t, w) in (("1 scene, R = 40", (tsdf1, weight1)), ("32 scenes, R = 40", (tsdf32, weight32)), ("1 scene, R = 120", (tsdf120, weight120))):
    pts, offs = perception.cloud_batch(t, w, SIZE)
    row(f"cloud count + emit, {name} ({len(pts)} points; with the D->H copy of the counts)", timed(lambda: perception.cloud_batch(t, w, SIZE)),
        t.shape[0] * (2 * 8 * t.shape[-1] ** 3) + 12 * len(pts))

host = torch.from_numpy(depth1)
row("upload of the six images, pageable host memory", timed(lambda: host.to(dev)), image_bytes)
pinned = host.pin_memory()
row("upload of the six images, pinned host memory", timed(lambda: pinned.to(dev, non_blocking=True)), image_bytes)
row("create_tsdf from host images (upload + new volume + integrate)", timed(lambda: perception.create_tsdf(SIZE, 40, depth1, intr, ext, dev)))

net = get_network("giga").to(dev)
net.load_state_dict(make_state_dict(7))
net.eval()
planner = VGNImplicit(None, "giga", net=net, best=True, force_detection=True, qual_th=0.6, out_th=0.1)
row("whole plan_from_depth (upload, fusion, network, grasp selection, D->H)", timed(lambda: planner.plan_from_depth(depth1, intr, ext, size=SIZE), warm=3))
vol = perception.create_tsdf(SIZE, 40, depth1, intr, ext, dev)
from types import SimpleNamespace  # noqa: E402
state = SimpleNamespace(tsdf=vol)
row("  of which the plan on the fused device volume", timed(lambda: planner(state)))
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    grasps, scores, _ = planner.plan_from_depth(depth1, intr, ext, size=SIZE)
log(f"  whole plan_from_depth call, wall: {(time.perf_counter() - t0) / 10 * 1e3:.2f} ms   ({len(grasps)} grasps)")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
