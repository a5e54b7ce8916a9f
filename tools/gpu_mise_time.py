"""Timing of the MISE value grid against the dense one: scene 70, weight seed 7, threshold 0.6 (the setting of
profiles/mesh/mesh_time.txt).  At 129^3 (resolution0 16, 3 steps), in one run: the dense value grid, the MISE rounds / points /
evaluation loop / to_dense fill, and the whole generate_mesh call both ways; at 257^3 (16 / 4) and 513^3 (32 / 4) MISE, and the
dense grid where one launch takes it.  HIP events around each piece (median of 20 repetitions after warm-up).  The evaluation loop
contains one copy of the list lengths to the host per round, so its event time includes the device's wait for the host.
Usage: python tools/gpu_mise_time.py [out.txt]"""
import statistics
import sys
import time

import torch

from giga_amd import synth
from giga_amd.generation import Generator3D
from giga_amd.mise import MISE
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


def row(name, t):
    med, lo, hi = t
    log(f"  {name:52s} {med * 1e3:10.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions)")


def wall(gen, x, reps):
    for _ in range(2):
        gen.generate_mesh({"inputs": x})
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        mesh = gen.generate_mesh({"inputs": x}, return_stats=False)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3, mesh


net = get_network("giga").to(dev)
net.load_state_dict(make_state_dict(7))
net.eval()
x = torch.from_numpy(synth.tsdf_batch(70, 1)).to(dev)
speedup = None
for res0, steps, dense_fits, normals in ((16, 3, True, True), (16, 4, True, False), (32, 4, False, False)):
    kw = dict(device=dev, threshold=0.6, resolution0=res0, upsampling_steps=steps, with_normals=normals)
    dense_gen, mise_gen = Generator3D(net, **kw), Generator3D(net, mise=True, **kw)
    n = mise_gen.grid_resolution()
    c = mise_gen.encode(x)
    lin = torch.from_numpy(mise_gen.mise_lin()).to(dev)
    iso = mise_gen._iso()
    state = {}

    def loop():
        m = MISE(res0, steps, iso, batch=1, device=dev, lin=lin)
        rounds = points = 0
        q = m.query()
        while q.shape[1]:
            rounds, points = rounds + 1, points + sum(m.counts)
            m.update(mise_gen.eval_points(m.points, c))
            q = m.query()
        state.update(m=m, rounds=rounds, points=points)

    loop()
    log(f"{n}^3 samples (resolution0 {res0}, {steps} upsampling steps), scene 70, weight seed 7, threshold 0.6: "
        f"MISE takes {state['rounds']} rounds and evaluates {state['points']} of {n ** 3} samples ({100.0 * state['points'] / n ** 3:.1f} %)")
    t_dense = None
    if dense_fits:
        t_dense = timed(lambda: dense_gen.value_grid(c))
        row("dense value grid (generic decoder, one launch)", t_dense)
    else:
        log(f"  dense value grid: not run ({n ** 3} decoder evaluations and a {n ** 3 * 12 / 1e9:.1f} GB point tensor in one launch)")
    t_loop = timed(loop)
    row("MISE evaluation loop (init, rounds of query / decoder / update)", t_loop)
    t_fill = timed(lambda: state["m"].to_dense())
    row("MISE to_dense fill", t_fill)
    if t_dense is not None:
        log(f"  MISE loop + fill against the dense grid: {(t_loop[0] + t_fill[0]) / t_dense[0]:.2f} x the time")
        if n == 129:
            speedup = t_dense[0] / (t_loop[0] + t_fill[0])
    reps = 10 if n == 129 else 3
    if dense_fits:
        ms, mesh = wall(dense_gen, x, reps)
        log(f"  whole generate_mesh call, dense, wall (normals {'on' if normals else 'off'}, with the copy of the mesh to the host): "
            f"{ms:.2f} ms, {len(mesh.vertices)} vertices")
    ms, mesh = wall(mise_gen, x, reps)
    log(f"  whole generate_mesh call, mise=True, wall (normals {'on' if normals else 'off'}, with the copy of the mesh to the host): "
        f"{ms:.2f} ms, {len(mesh.vertices)} vertices")
    del state, dense_gen, mise_gen
    torch.cuda.empty_cache()
log("recommendation at 129^3: " + ("mise=True is faster here" if speedup and speedup > 1 else "mise=True is NOT faster here; use it for "
    "the reference's mesh (it skips components smaller than a coarse cell) and for grids beyond 129^3") +
    f" (dense / (loop + fill) = {speedup:.2f}); the default stays the dense grid")
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
