"""Timing of giga_mesh_collide (csrc/giga_collide.hip): 32 scenes x 12 candidate bodies = 384 bodies, the 66 pairs inside every
scene = 2112 pairs in one call, icospheres of 1280 (about 10^3) and 5120 (about 10^4) triangles, for packed-style placements
(random positions on the reference's 0.14 m square: most boxes are disjoint or overlap a little) and for the case the culling
helps least (12 concentric spheres per scene: every pair's boxes are nested, nearly all triangles survive and no pair is decided
early).  Beside it the time of a whole `generate_packed_scenes` batch of 32 scenes, whose difference to the collision call is the
host's draws, transformation, packing and upload.  Each bracketed by HIP events (median of 20 repetitions after warm-up, one process).
Usage: timeout -k 10 900 python tools/gpu_collide_time.py [out.txt]   (one GPU step: run it under its own time limit, chained with &&)"""
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import collide_emu as cemu  # noqa: E402  (mesh generators, .obj writer)
from giga_amd import collision, scenes  # noqa: E402

dev = torch.device("cuda:0")
lines = []
SCENES, PER_SCENE = 32, 12
PAIRS = np.concatenate([scenes.ATTEMPT_PAIRS + PER_SCENE * k for k in range(SCENES)])


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
    log(f"  {name:84s} {med * 1e3:12.1f} us   (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}; HIP events, 20 repetitions){extra}")


def packed_bodies(subdiv, seed):
    rng = np.random.default_rng([seed, subdiv])
    out = []
    for _ in range(SCENES * PER_SCENE):
        r = 0.03 * rng.uniform(0.7, 0.9)
        out.append(cemu.icosphere(np.r_[rng.uniform(0.08, 0.22, 2), 0.052 + r], r, subdiv))
    return out


def concentric_bodies(subdiv):
    # radii fall by 3 % a step, more than the gap between an icosphere of subdivision >= 3 and its inscribed sphere
    one = [cemu.icosphere((0.15, 0.15, 0.1), 0.04 * 0.97 ** k, subdiv) for k in range(PER_SCENE)]
    return one * SCENES


def on_device(bodies):
    return [(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)) for v, f in bodies]


log(f"giga_mesh_collide: {SCENES} scenes x {PER_SCENE} bodies, {len(PAIRS)} pairs per call (bodies already on the device)")
for subdiv in (3, 4):
    for name, bodies in (("packed-style placements", packed_bodies(subdiv, 0)), ("concentric: boxes nested, no pair decided early", concentric_bodies(subdiv))):
        tri = len(bodies[0][1])
        meshes = on_device(bodies)
        hits = int(collision.mesh_collide(meshes, PAIRS, containment=False, device=dev).sum())
        row(f"surface test, {tri} triangles per body, {name}", timed(lambda: collision.mesh_collide(meshes, PAIRS, containment=False, device=dev)),
            f"   {hits} of {len(PAIRS)} pairs intersect")
        if name.startswith("packed"):
            row(f"... with the two containment queries per pair, {tri} triangles per body", timed(lambda: collision.mesh_collide(meshes, PAIRS, containment=True, device=dev)))

with tempfile.TemporaryDirectory() as tmp:
    for subdiv in (3, 4):
        root = os.path.join(tmp, f"spheres{subdiv}")
        os.makedirs(root)
        for k, r in enumerate((0.025, 0.03, 0.035)):
            cemu.write_obj(os.path.join(root, f"sphere{k}.obj"), *cemu.icosphere((0, 0, 0), r, subdiv))
        objects = scenes.ObjectSet(root)
        kept = sum(len(s) for s in scenes.generate_packed_scenes(objects, SCENES, seed=0, batch=SCENES, device=dev))
        row(f"generate_packed_scenes, one batch of {SCENES} scenes, {20 * 4 ** subdiv} triangles per object (host work included)",
            timed(lambda: scenes.generate_packed_scenes(objects, SCENES, seed=0, batch=SCENES, device=dev)), f"   {kept} objects kept")
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
