"""Time giga_amd.mesh.simplify_mesh on the device (EXPERIMENTS.md):

    python tools/gpu_simplify_time.py [--out FILE.npz]

Meshes: icospheres of 20 480 and 81 920 faces (5 and 6 subdivisions, 1e-4 noise) and the mesh Generator3D gives at 129^3 for a
synthetic scene (synthetic weights, seed 7), each at a tenth of its faces, agressiveness 5; one mesh alone and a batch of 8 copies.
Prints per case the device milliseconds (median of 3 calls after one warm-up; the call is synchronous), iterations, rounds,
repeated passes and kernel launches (giga_launch_count), hence milliseconds and launches per round.  --out stores the meshes
(NAME_vertices, NAME_faces, NAME_target) for `python tools/make_simplify_goldens.py --time FILE.npz`, which times the reference's
Simplify.h on the same arrays on the CPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from giga_amd import _capi, networks, synth, weights  # noqa: E402
from giga_amd.generation import Generator3D  # noqa: E402
from giga_amd.mesh import simplify_mesh  # noqa: E402


def icosphere(subdivisions, radius=0.4, noise=1e-4, seed=1):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = v[a] + v[b]
                v.append(m / np.linalg.norm(m))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    v = np.array(v) * radius + np.random.default_rng(seed).normal(0.0, noise, (len(v), 3))
    return v.astype(np.float32), np.array(f, np.int32)


def generator_mesh(dev):
    net = networks.get_network("giga")
    net.load_state_dict(weights.make_state_dict(7))
    net = net.to(dev).eval()
    mesh = Generator3D(net, device=dev, threshold=0.6).generate_mesh({"inputs": torch.from_numpy(synth.tsdf_batch(40, 1))},
                                                                     return_stats=False)
    return mesh.vertices, mesh.faces.astype(np.int32)


def timed(v, f, target, copies):
    L = _capi.lib()
    vs, fs = torch.cat([v] * copies), torch.cat([f] * copies)
    counts = [(len(v), len(f))] * copies
    best, stats, launches = [], {}, 0
    for k in range(4):
        torch.cuda.synchronize()
        n0, t0 = L.giga_launch_count(), time.perf_counter()
        out = simplify_mesh(vs, fs, target, 5., counts=counts, stats=stats)
        torch.cuda.synchronize()
        if k:
            best.append(time.perf_counter() - t0)
        launches = L.giga_launch_count() - n0
    return 1e3 * float(np.median(best)), stats, launches, int(out[2][0, 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    meshes = {"ico5": icosphere(5), "ico6": icosphere(6), "gen129": generator_mesh(dev)}
    store = {}
    for name, (v, f) in meshes.items():
        target = len(f) // 10
        store[name + "_vertices"], store[name + "_faces"], store[name + "_target"] = v, f, np.int64(target)
        tv, tf = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
        for copies in (1, 8):
            ms, stats, launches, faces = timed(tv, tf, target, copies)
            rounds = max(stats["rounds"])
            print(f"{name} x{copies}: {len(f)} faces -> {faces} (target {target}): {ms:.1f} ms, iterations {stats['iterations'][0]}, "
                  f"rounds {rounds}, repeated passes {stats['repeated passes'][0]}, list rebuilds {stats['list rebuilds'][0]}, "
                  f"launches {launches} ({launches / max(rounds, 1):.2f} per round), {1e3 * ms / max(rounds, 1):.1f} us per round",
                  flush=True)
    if args.out:
        np.savez_compressed(args.out, **store)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
