"""Write tests/golden/g20_simplify.npz: quadric edge-collapse fixtures from the reference's own utils/libsimplify/Simplify.h.

    python tools/make_simplify_goldens.py

Needs the reference checkout (oracle/ref_bootstrap.py: REFERENCE_SRC) and g++.  The tool writes a few-line driver of its own into a
TEMPORARY directory; the driver includes the reference's Simplify.h by -I, fills Simplify::vertices / Simplify::triangles with
VALUE-INITIALISED records (`Vertex()`, `Triangle()`), calls `Simplify::simplify_mesh(target, agressiveness)` and writes the arrays
back.  It is compiled there with g++ -O2 and run; nothing compiled or copied from the reference enters the repository, only arrays
are stored.  (The reference's Cython wrapper, simplify_mesh.pyx, cannot serve: its struct literals leave members unset and its
result changes with the call that went before -- DESIGN.md section 3r.)

The tool refuses to write when two runs of the driver disagree or when tests/simplify_emu.py (sequential form, and the round
schedule in both winner orders) disagrees with the driver.  For every case NAME of `names`:

  NAME_vertices_in   float32 (V,3)       NAME_faces_in   int32 (F,3)
  NAME_target        int64               NAME_agressiveness  float64
  NAME_vertices      float64 (V',3)      NAME_faces      int32 (F',3)      the driver's output
  NAME_cpu_seconds   float64             CPU time of simplify_mesh inside the driver on the machine that ran the tool
  NAME_stats         int64 [iterations, rounds, repeated passes, longest pass]   of the round schedule (tests/simplify_emu.py)

`python tools/make_simplify_goldens.py --time FILE.npz` only times the driver on the meshes of FILE.npz (keys NAME_vertices,
NAME_faces, NAME_target; agressiveness 5) and prints the CPU seconds: the CPU side of tools/gpu_simplify_time.py."""
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_emu  # noqa: E402
import simplify_emu  # noqa: E402

DRIVER = r"""
#include "Simplify.h"
#include <ctime>
int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "rb");
    int nv, nf, target; double aggr;
    if (!in || fread(&nv, 4, 1, in) != 1 || fread(&nf, 4, 1, in) != 1 || fread(&target, 4, 1, in) != 1 || fread(&aggr, 8, 1, in) != 1) return 1;
    std::vector<double> v(3 * (size_t)nv); std::vector<int> f(3 * (size_t)nf);
    if (nv && fread(v.data(), 8, v.size(), in) != v.size()) return 1;
    if (nf && fread(f.data(), 4, f.size(), in) != f.size()) return 1;
    fclose(in);
    for (int i = 0; i < nv; ++i) { Simplify::Vertex r = Simplify::Vertex(); r.p.x = v[3 * i]; r.p.y = v[3 * i + 1]; r.p.z = v[3 * i + 2]; Simplify::vertices.push_back(r); }
    for (int i = 0; i < nf; ++i) { Simplify::Triangle r = Simplify::Triangle(); for (int j = 0; j < 3; ++j) r.v[j] = f[3 * i + j]; Simplify::triangles.push_back(r); }
    const clock_t t0 = clock();
    Simplify::simplify_mesh(target, aggr);
    const double seconds = double(clock() - t0) / CLOCKS_PER_SEC;
    FILE* out = fopen(argv[2], "wb");
    nv = (int)Simplify::vertices.size(); nf = (int)Simplify::triangles.size();
    fwrite(&nv, 4, 1, out); fwrite(&nf, 4, 1, out); fwrite(&seconds, 8, 1, out);
    for (int i = 0; i < nv; ++i) { double p[3] = {Simplify::vertices[i].p.x, Simplify::vertices[i].p.y, Simplify::vertices[i].p.z}; fwrite(p, 8, 3, out); }
    for (int i = 0; i < nf; ++i) fwrite(Simplify::triangles[i].v, 4, 3, out);
    fclose(out);
    return 0;
}
"""


def build_driver(tmp):
    from oracle import ref_bootstrap
    inc = os.path.join(ref_bootstrap.REFERENCE_SRC, "vgn", "ConvONets", "utils", "libsimplify")
    src, exe = os.path.join(tmp, "driver.cpp"), os.path.join(tmp, "driver")
    with open(src, "w") as fh:
        fh.write(DRIVER)
    subprocess.run(["g++", "-O2", "-w", "-I" + inc, src, "-o", exe], check=True)
    return exe


def run_driver(exe, tmp, vertices, faces, target, agressiveness):
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    v = np.ascontiguousarray(vertices, dtype=np.float64)
    f = np.ascontiguousarray(faces, dtype=np.int32)
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<iiid", len(v), len(f), int(target), float(agressiveness)))
        fh.write(v.tobytes())
        fh.write(f.tobytes())
    subprocess.run([exe, fin, fout], check=True)
    raw = open(fout, "rb").read()
    nv, nf, seconds = struct.unpack_from("<iid", raw)
    ov = np.frombuffer(raw, np.float64, 3 * nv, 16).reshape(nv, 3).copy()
    of = np.frombuffer(raw, np.int32, 3 * nf, 16 + 24 * nv).reshape(nf, 3).copy()
    return ov, of, seconds


# ---- meshes --------------------------------------------------------------------------------------------------------------
def tetrahedron():
    v = np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float32) * np.float32(0.25)
    return v, np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)


def octahedron():
    v = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32) * np.float32(0.3)
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return v, np.array(f, np.int32)


def icosphere(subdivisions, radius=0.4, noise=0.0, seed=0):
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
    v = np.array(v) * radius
    if noise:
        v = v + np.random.default_rng(seed).normal(0.0, noise, v.shape)
    return v.astype(np.float32), np.array(f, np.int32)


def torus(n=24, m=24):
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    u, w = 2 * np.pi * i / n, 2 * np.pi * j / m
    r = 0.12 * (1 + 0.25 * np.sin(3 * u) * np.cos(2 * w))
    v = np.stack(((0.3 + r * np.cos(w)) * np.cos(u), (0.3 + r * np.cos(w)) * np.sin(u), r * np.sin(w)), -1).reshape(-1, 3)
    idx = lambda a, b: (a % n) * m + (b % m)
    f = []
    for a in range(n):
        for b in range(m):
            f += [(idx(a, b), idx(a + 1, b), idx(a + 1, b + 1)), (idx(a, b), idx(a + 1, b + 1), idx(a, b + 1))]
    return v.astype(np.float32), np.array(f, np.int32)


def cap(n_faces=808):
    """The n_faces highest faces of a 3-subdivision icosphere (in their original order), vertices renumbered: an open mesh."""
    v, f = icosphere(3, noise=1e-4, seed=3)
    height = v[f].astype(np.float64).mean(1)[:, 2]
    keep = np.sort(np.argsort(-height, kind="stable")[:n_faces])
    f = f[keep]
    used = np.unique(f)
    new = np.full(len(v), -1, np.int32)
    new[used] = np.arange(len(used), dtype=np.int32)
    return v[used], new[f]


def mc_balls(n, balls):
    c = np.arange(n, dtype=np.float64) / (n - 1) - 0.5
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    field = np.full((n, n, n), -np.inf)
    for (cx, cy, cz), r in balls:
        field = np.maximum(field, r - np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2))
    return mesh_emu.marching_cubes(field.astype(np.float32), 0.0, 1.1)         # (positive inside, like the occupancy logits)


def with_unreferenced_vertex():
    v, f = icosphere(1, noise=1e-4, seed=5)
    k = 17
    v = np.concatenate((v[:k], np.array([[0.01, 0.02, 0.03]], np.float32), v[k:]))
    return v, np.where(f >= k, f + 1, f).astype(np.int32)


def cases():
    yield "tetra_2", tetrahedron(), 2, 5.0
    yield "octa_4", octahedron(), 4, 5.0
    ico = icosphere(2, noise=1e-4, seed=1)
    for t in (160, 32, 6):
        yield f"ico2_{t}", ico, t, 5.0
    tor = torus()
    for t in (576, 114, 7):
        yield f"torus_{t}", tor, t, 5.0
    cp = cap()
    for t in (404, 80, 7):
        yield f"cap_{t}", cp, t, 5.0
    sph = mc_balls(17, [((0.0, 0.0, 0.0), 0.3)])
    for d in (2, 10):
        yield f"mc17_f{d}", sph, len(sph[1]) // d, 5.0
    two = mc_balls(33, [((-0.1, 0.0, 0.0), 0.16), ((0.12, 0.04, 0.0), 0.12)])
    for d in (2, 10):
        yield f"mc33_f{d}", two, len(two[1]) // d, 5.0
    yield "unref_40", with_unreferenced_vertex(), 40, 7.0
    yield "ico2_keep", ico, 320, 7.0                           # target >= F: only the final compaction
    yield "unref_keep", with_unreferenced_vertex(), 1000, 5.0
    yield "ico1_0", icosphere(1, noise=1e-4, seed=5), 0, 7.0


def time_only(path):
    data = np.load(path)
    names = sorted(k[:-len("_vertices")] for k in data.files if k.endswith("_vertices"))
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name in names:
            v, f, t = data[name + "_vertices"], data[name + "_faces"], int(data[name + "_target"])
            best = min(run_driver(exe, tmp, v, f, t, 5.0)[2] for _ in range(3))
            ov, of, _ = run_driver(exe, tmp, v, f, t, 5.0)
            print(f"{name}: faces {len(f)} -> {len(of)} (target {t}), driver CPU {1e3 * best:.2f} ms", flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--time":
        return time_only(sys.argv[2])
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        for name, (v, f), target, aggr in cases():
            assert v.dtype == np.float32 and f.dtype == np.int32
            ov, of, seconds = run_driver(exe, tmp, v, f, target, aggr)
            ov2, of2, _ = run_driver(exe, tmp, v, f, target, aggr)
            if ov.tobytes() != ov2.tobytes() or of.tobytes() != of2.tobytes():
                raise SystemExit(f"{name}: two runs of the driver disagree; nothing written")
            ev, ef = simplify_emu.simplify(v, f, target, aggr)
            if ev.tobytes() != ov.tobytes() or ef.tobytes() != of.tobytes():
                raise SystemExit(f"{name}: the sequential emulator disagrees with the driver ({len(ef)} faces against {len(of)}); "
                                 "nothing written")
            stats = {}
            for order in ("ascending", "descending"):
                rv, rf = simplify_emu.simplify_rounds(v, f, target, aggr, order=order, stats=stats)
                if rv.tobytes() != ov.tobytes() or rf.tobytes() != of.tobytes():
                    raise SystemExit(f"{name}: the round emulator ({order}) disagrees with the driver; nothing written")
            print(f"{name}: {len(v)} vertices, {len(f)} faces -> {len(ov)}, {len(of)} (target {target}); iterations "
                  f"{stats['iterations']}, rounds {stats['rounds']}, repeated passes {stats['repeats']}, longest pass "
                  f"{stats['longest_pass']}; driver {1e3 * seconds:.2f} ms", flush=True)
            names.append(name)
            out[name + "_vertices_in"], out[name + "_faces_in"] = v, f
            out[name + "_target"], out[name + "_agressiveness"] = np.int64(target), np.float64(aggr)
            out[name + "_vertices"], out[name + "_faces"] = ov, of
            out[name + "_cpu_seconds"] = np.float64(seconds)
            out[name + "_stats"] = np.array([stats["iterations"], stats["rounds"], stats["repeats"], stats["longest_pass"]], np.int64)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "g20_simplify.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
