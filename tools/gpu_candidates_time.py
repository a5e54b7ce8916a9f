"""Timing of giga_tsdf_cloud_emit_oriented beside giga_tsdf_cloud_emit, and of giga_grasp_candidates (csrc/giga_tsdf.hip,
csrc/giga_candidates.hip): 32 scenes of spheres on a table, six rendered 480x640 views each, fused at resolution 120.  The two emit
calls read the workspace of one giga_tsdf_cloud_count; the candidates are drawn from the oriented cloud with K = 120, Y = 6 inside
the reference's bounds.  Only the library call lies between the HIP events (buffers and workspaces are allocated before); median
of 20 repetitions after warm-up, one process, the three calls interleaved.
Usage: timeout -k 10 600 python tools/gpu_candidates_time.py [out.txt]   (one GPU step: run it under its own time limit)"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collide_emu as cemu  # noqa: E402  (mesh generators)
from giga_amd import _capi, candidates, perception, render, scenes  # noqa: E402

dev = torch.device("cuda:0")
lines = []
B, R, SIZE, K, Y = 32, 120, 0.3, 120, 6


def log(s):
    print(s, flush=True)
    lines.append(s)


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def scene(seed):
    rng = np.random.default_rng(seed)
    table = scenes.table_mesh(SIZE)
    verts, faces, base = [table[0]], [table[1]], len(table[0])
    for _ in range(4):
        r = 0.03 * rng.uniform(0.7, 1.2)
        v, f = cemu.icosphere(np.r_[rng.uniform(0.07, 0.23, 2), 0.05 + r * rng.uniform(0.6, 1.0)], r, 3)
        verts.append(v.astype(np.float32))
        faces.append(f.astype(np.int32) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(faces)


meshes = [scene(s) for s in range(B)]
intrinsic = render.sim_intrinsic()
views = [candidates.scene_views(0, s, SIZE) for s in range(B)]
depth, offs = render.render_depth_batch(meshes, intrinsic, views, device=dev)
tsdf, weight, _ = perception.fuse_scenes(SIZE, R, [depth[offs[b]:offs[b + 1]] for b in range(B)], intrinsic, views, dev)
del depth
ws = _capi.workspace("giga_tsdf_cloud", dev, B, R)
counts = torch.empty(B, dtype=torch.int32, device=dev)
_capi.call("giga_tsdf_cloud_count", dev, tsdf, weight, B, R, ws, ws.numel(), counts)
offsets = np.concatenate(([0], np.cumsum(counts.cpu().numpy().astype(np.int64)))).astype(np.int32)
n = int(offsets[-1])
points, normals = torch.empty((n, 3), device=dev), torch.empty((n, 3), device=dev)
plain = torch.empty((n, 3), device=dev)
lower, upper = candidates.workspace_bounds(SIZE, scenes.TABLE_HEIGHT)
table = candidates.yaw_table(Y)
ids = np.arange(B, dtype=np.uint32)
pos = torch.zeros((B, K, 3), dtype=torch.float64, device=dev)
quat = torch.zeros((B, K, Y, 4), dtype=torch.float64, device=dev)
index = torch.zeros((B, K), dtype=torch.int32, device=dev)
eligible = torch.zeros(B, dtype=torch.int32, device=dev)
cws = _capi.workspace("giga_grasp_candidates", dev, B, n, Y)
calls = {
    "giga_tsdf_cloud_emit": lambda: _capi.call("giga_tsdf_cloud_emit", dev, tsdf, weight, B, R, SIZE, ws, ws.numel(), plain, n, None),
    "giga_tsdf_cloud_emit_oriented": lambda: _capi.call("giga_tsdf_cloud_emit_oriented", dev, tsdf, weight, B, R, SIZE, ws, ws.numel(), points,
                                                        normals, n, None),
    "giga_grasp_candidates": lambda: _capi.call("giga_grasp_candidates", dev, points, normals, offsets, ids, B, K, lower, upper, 0.05, 0.1,
                                                table, Y, 0, pos, quat, index, eligible, cws, cws.numel()),
}
for _ in range(3):
    for fn in calls.values():
        fn()
times = {name: [] for name in calls}
for _ in range(20):
    for name, fn in calls.items():
        times[name].append(event_ms(fn))
assert torch.equal(plain, points)
volume = 2 * 4 * B * R ** 3                     # tsdf and weight, once
log(f"{B} scenes, R = {R}: {n} crossings ({n // B} a scene), {int(eligible.sum())} eligible inside the bounds; K = {K}, Y = {Y}")
log(f"  state read once by either emit call: {volume / 1e6:.1f} MB; points {12 * n / 1e6:.2f} MB, normals {12 * n / 1e6:.2f} MB written; "
    f"{48 * 4 * n / 1e6:.1f} MB of scattered 4-byte reads for the normals")
log(f"  candidates: {24 * n / 1e6:.2f} MB read, {4 * int(eligible.sum()) / 1e6:.2f} MB list written, {B * K * (24 + 4 + 32 * Y) / 1e6:.3f} MB results written")
for name, t in times.items():
    log(f"  {name:32s} {statistics.median(t) * 1e3:10.1f} us   (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}; HIP events, 20 repetitions)")
ratio = statistics.median(times["giga_tsdf_cloud_emit_oriented"]) / statistics.median(times["giga_tsdf_cloud_emit"])
log(f"  oriented / plain = {ratio:.2f}")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
