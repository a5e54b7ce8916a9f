"""Write tests/golden/g19_mise.npz: MISE fixtures from the reference's own libmise.

    python tools/make_mise_goldens.py

Needs the reference checkout (oracle/ref_bootstrap.py: REFERENCE_SRC), Cython and g++.  The reference's utils/libmise/mise.pyx is
cythonized and compiled into a TEMPORARY directory (nothing compiled or copied from the reference enters the repository) and
driven as conv_onet/generation.py:128-141 drives it, with lookups into a float32 field in place of the network.  Only arrays are
stored; for every case NAME of `names`:

  NAME_field      float32 (R+1)^3, R = resolution0 << depth
  NAME_setup      int64 [resolution0, depth]
  NAME_threshold  float64
  NAME_rounds     int32: the query sets of all rounds as sorted linear indices (i (R+1) + j) (R+1) + k, back to back
  NAME_sizes      int64: the length of every round
  NAME_dense      float32 (R+1)^3: to_dense()

Cases (x = index / R - 0.5 per axis, |x| the Euclidean norm):
  sphere43, sphere42   0.3 - |x|, resolution0 4, depth 3 and 2
  slab43               max(0.3 - |x|, 0.011 - |x0 - 0.37|), 4 / 3: five rounds, a leaf left alone in one round is subdivided later
  ball43               0.02 - |x - 0.03|, 4 / 3: smaller than a coarse cell, one round, nothing positive
  sphere32             0.3 - |x|, resolution0 3 (no power of two), depth 2
  sphere41             0.3 - |x|, depth 1
  positive22, negative22   constant fields, one round
  plane42              the integer field i - 8, 4 / 2: equal to the threshold on the whole lattice plane i = 8
  faces42              0.6 - |x|, 4 / 2: the surface cuts the six boundary faces
"""
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mise_emu  # noqa: E402


def reference_mise(tmp):
    from oracle import ref_bootstrap
    src = os.path.join(ref_bootstrap.REFERENCE_SRC, "vgn", "ConvONets", "utils", "libmise", "mise.pyx")
    cpp = os.path.join(tmp, "mise.cpp")
    subprocess.run([sys.executable, "-m", "cython", "--cplus", "-3", src, "-o", cpp], check=True)
    lib = os.path.join(tmp, "mise" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-w", "-I" + sysconfig.get_paths()["include"], "-I" + np.get_include(), cpp,
                    "-o", lib], check=True)
    spec = importlib.util.spec_from_file_location("mise", lib)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.MISE


def coords(res):
    c = np.arange(res + 1, dtype=np.float64) / res - 0.5
    return np.meshgrid(c, c, c, indexing="ij")


def sphere(res, radius, centre=0.0):
    x, y, z = coords(res)
    return (radius - np.sqrt((x - centre) ** 2 + (y - centre) ** 2 + (z - centre) ** 2)).astype(np.float32)


def slab(res):
    x, y, z = coords(res)
    return np.maximum(0.3 - np.sqrt(x * x + y * y + z * z), 0.011 - np.abs(x - 0.37)).astype(np.float32)


def cases():
    yield "sphere43", 4, 3, 0.0, sphere(32, 0.3)
    yield "sphere42", 4, 2, 0.0, sphere(16, 0.3)
    yield "slab43", 4, 3, 0.0, slab(32)
    yield "ball43", 4, 3, 0.0, sphere(32, 0.02, 0.03)
    yield "sphere32", 3, 2, 0.0, sphere(12, 0.3)
    yield "sphere41", 4, 1, 0.0, sphere(8, 0.3)
    yield "positive22", 2, 2, 0.25, np.full((9, 9, 9), 1.0, np.float32)
    yield "negative22", 2, 2, 0.25, np.full((9, 9, 9), -1.0, np.float32)
    yield "plane42", 4, 2, 0.0, (np.arange(17, dtype=np.float32)[:, None, None] - 8) * np.ones((17, 17, 17), np.float32)
    yield "faces42", 4, 2, 0.0, sphere(16, 0.6)


def run_reference(MISE, field, res0, depth, threshold):
    """generation.py:128-141 with a lookup for eval_points."""
    m = MISE(res0, depth, threshold)
    n = m.resolution + 1
    rounds = []
    points = m.query()
    while points.shape[0] != 0:
        rounds.append(np.sort((points[:, 0] * n + points[:, 1]) * n + points[:, 2]).astype(np.int32))
        values = field[points[:, 0], points[:, 1], points[:, 2]].astype(np.float64)
        m.update(points, values)
        points = m.query()
    return rounds, m.to_dense()


def main():
    out, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        MISE = reference_mise(tmp)
        for name, res0, depth, thr, field in cases():
            rounds, dense = run_reference(MISE, field, res0, depth, thr)
            assert not np.isnan(dense).any() and np.array_equal(dense.astype(np.float32).astype(np.float64), dense)
            emu_rounds, emu_dense = mise_emu.run(field, res0, depth, thr)
            same = len(rounds) == len(emu_rounds) and all(np.array_equal(a, b) for a, b in zip(rounds, emu_rounds)) and \
                emu_dense.tobytes() == dense.astype(np.float32).tobytes()
            print(name, "sizes", [len(r) for r in rounds], "evaluated", sum(len(r) for r in rounds), "of", field.size,
                  "emulator agrees" if same else "EMULATOR DIFFERS")
            names.append(name)
            out[name + "_field"] = field
            out[name + "_setup"] = np.array([res0, depth], np.int64)
            out[name + "_threshold"] = np.float64(thr)
            out[name + "_rounds"] = np.concatenate(rounds) if rounds else np.zeros(0, np.int32)
            out[name + "_sizes"] = np.array([len(r) for r in rounds], np.int64)
            out[name + "_dense"] = dense.astype(np.float32)
    out["names"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "g19_mise.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
