"""Timing of Generator3D.generate_mesh at the reference's default setting (129^3 samples): encode, value grid, marching-cubes
count and emit, vertex normals, each bracketed by HIP events (median of the repetitions after warm-up), and the wall time of
the whole call.  Usage: python tools/gpu_mesh_time.py [out.txt]"""
import statistics
import sys
import time

import torch

from giga_amd import _capi, synth
from giga_amd.convonet import _planes_to_nhwc
from giga_amd.generation import Generator3D
from giga_amd.networks import get_network
from giga_amd.weights import make_state_dict

dev = torch.device("cuda:0")
lines = []


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


net = get_network("giga").to(dev)
net.load_state_dict(make_state_dict(7))
net.eval()
gen = Generator3D(net, device=dev, threshold=0.6, with_normals=True)
n = gen.grid_resolution()
x = torch.from_numpy(synth.tsdf_batch(70, 1)).to(dev)
c = gen.encode(x)
grid = gen.value_grid(c)
iso, box = gen._iso(), 1 + gen.padding
L = _capi.lib()
ws = torch.empty(L.giga_mesh_workspace_bytes(1, n, n, n), dtype=torch.uint8, device=dev)
counts = torch.zeros((1, 2), dtype=torch.int32, device=dev)


def count():
    _capi.check(L.giga_mesh_count(_capi.ptr(grid), 1, n, n, n, iso, _capi.ptr(ws), ws.numel(), _capi.ptr(counts),
                                  _capi.stream_ptr(dev)), "giga_mesh_count")


count()
nv, nt = counts.cpu()[0].tolist()
vertices = torch.empty((nv, 3), device=dev)
triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)


def emit():
    _capi.check(L.giga_mesh_emit(_capi.ptr(grid), 1, n, n, n, iso, box, _capi.ptr(ws), ws.numel(), _capi.ptr(vertices), nv,
                                 _capi.ptr(triangles), nt, None, _capi.stream_ptr(dev)), "giga_mesh_emit")


emit()
nhwc = _planes_to_nhwc(c, "fp32")
log(f"generate_mesh, {n}^3 samples ({(n + 1) ** 3} cells), scene 70, weight seed 7, threshold 0.6: {nv} vertices, {nt} triangles")
for name, fn in (("encode (fp32)", lambda: gen.encode(x)), ("value grid (generic decoder, one launch)", lambda: gen.value_grid(c)),
                 ("marching cubes: count (classify + scans)", count), ("marching cubes: emit", emit),
                 ("vertex normals (point gradient)", lambda: gen._normals_on_device(vertices, nhwc))):
    med, lo, hi = timed(fn)
    log(f"  {name:45s} {med * 1e3:9.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions)")
log(f"  count reads {n ** 3 * 4 / 1e6:.1f} MB of samples and writes {(n + 1) ** 3 * 4 / 1e6:.1f} MB of cell words: back-to-back repetitions keep this "
    "17-MB working set in the 256-MB Infinity Cache, as it is inside generate_mesh (the decoder has just written the grid); a caller "
    "with a cold grid reads it from HBM and will not see these figures")
for _ in range(3):
    gen.generate_mesh({"inputs": x})
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(10):
    gen.generate_mesh({"inputs": x})
torch.cuda.synchronize()
log(f"  whole generate_mesh call, wall (with the copy of the mesh to the host): {(time.perf_counter() - t0) / 10 * 1e3:.2f} ms")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
