"""Write tests/golden/g17_eval.npz: mesh-evaluation fixtures from the reference's own vgn.ConvONets.eval.

    python tools/make_eval_goldens.py

Needs the reference checkout (oracle/ref_bootstrap.py: REFERENCE_SRC), cython, gcc and g++.  The reference's two Cython
extensions (utils/libkdtree/pykdtree/kdtree.pyx with _kdtree_core.c, utils/libmesh/triangle_hash.pyx) are compiled into a
TEMPORARY directory and loaded under their dotted names; nothing compiled or copied from the reference enters the repository.
Only arrays are stored.  The inputs are regenerated from seeds by tests/eval_emu.py (`case_inputs`); per case (A, B: the two
meshes of g16_mesh.npz, each against itself scaled by 1.02 and shifted by 0.003) the fixture holds

  seed, checksum            the seed that passed the two shares below, sha256 of the regenerated inputs
  comp_* / acc_*            distance_p2p(target -> prediction) / (prediction -> target): dist (float32), idx, normal dot products
  metric_keys, metrics      the dictionary MeshEvaluator.eval_pointcloud returns
  contains_512 / _128       check_mesh_contains for 20 000 uniform points in [-0.5, 0.5]^3 (bit-packed), hash_resolution 512 / 128
  iou                       compute_iou(contains_512, |p| < 0.3)
  near_tie_share            share of source points whose second-nearest target is within 1e-6 (relative) of the nearest
  near_threshold            number of points within 1e-6 (relative) of the 1 %, 1.5 %, 2 % thresholds
  kdtree_vs_float64         max relative difference of the reference's distances from a float64 brute force
  *_reference_seconds       the reference's CPU time for the two queries / the containment test
"""
import importlib.machinery
import importlib.util
import os
import subprocess
import sys
import sysconfig
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_emu  # noqa: E402


def _load(path, dotted):
    loader = importlib.machinery.ExtensionFileLoader(dotted, path)
    spec = importlib.util.spec_from_file_location(dotted, path, loader=loader)
    mod = importlib.util.module_from_spec(spec)
    loader.exec_module(mod)
    sys.modules[dotted] = mod
    return mod


def reference_eval(tmp):
    """compile the two extensions into `tmp`, register them, and import vgn.ConvONets.eval"""
    from oracle import ref_bootstrap
    ref_bootstrap.install()
    utils = os.path.join(ref_bootstrap.REFERENCE_SRC, "vgn", "ConvONets", "utils")
    inc = ["-I" + sysconfig.get_paths()["include"], "-I" + np.get_include()]
    ext = sysconfig.get_config_var("EXT_SUFFIX")
    kd_src = os.path.join(utils, "libkdtree", "pykdtree")
    kd_c, kd_so = os.path.join(tmp, "kdtree.c"), os.path.join(tmp, "kdtree" + ext)
    subprocess.run(["cython", "-3", os.path.join(kd_src, "kdtree.pyx"), "-o", kd_c], check=True)
    subprocess.run(["gcc", "-O2", "-shared", "-fPIC", "-std=c99", "-w"] + inc + [kd_c, os.path.join(kd_src, "_kdtree_core.c"), "-o", kd_so],
                   check=True)
    th_cpp, th_so = os.path.join(tmp, "triangle_hash.cpp"), os.path.join(tmp, "triangle_hash" + ext)
    subprocess.run(["cython", "-3", "--cplus", os.path.join(utils, "libmesh", "triangle_hash.pyx"), "-o", th_cpp], check=True)
    subprocess.run(["g++", "-O2", "-shared", "-fPIC", "-w"] + inc + [th_cpp, "-o", th_so], check=True)
    _load(kd_so, "vgn.ConvONets.utils.libkdtree.pykdtree.kdtree")
    _load(th_so, "vgn.ConvONets.utils.libmesh.triangle_hash")
    import vgn.ConvONets.eval as ref_eval
    return ref_eval


def run_case(ref_eval, g16, name, seed):
    inp = eval_emu.case_inputs(g16, name, seed)
    mesh = types.SimpleNamespace(vertices=inp["v"], faces=inp["f"])
    out = {"seed": np.int64(seed), "checksum": eval_emu.checksum(inp)}
    t0 = time.perf_counter()
    comp, comp_dot = ref_eval.distance_p2p(inp["tgt"], inp["n_tgt"], inp["pred"], inp["n_pred"])
    acc, acc_dot = ref_eval.distance_p2p(inp["pred"], inp["n_pred"], inp["tgt"], inp["n_tgt"])
    out["nn_reference_seconds"] = np.float64(time.perf_counter() - t0)
    from vgn.ConvONets.utils.libkdtree import KDTree
    ci = KDTree(inp["pred"]).query(inp["tgt"])[1]
    ai = KDTree(inp["tgt"]).query(inp["pred"])[1]
    share, near, worst = 0.0, 0, 0.0
    for d, i, src, tgt in ((comp, ci, inp["tgt"], inp["pred"]), (acc, ai, inp["pred"], inp["tgt"])):
        d64, i64, second = eval_emu.nn_brute(src, tgt)
        tie = eval_emu.near_tie(d64, second)
        assert np.array_equal(i64[~tie], np.asarray(i, np.int64)[~tie])
        share = max(share, float(tie.mean()))
        worst = max(worst, float((np.abs(d.astype(np.float64) - d64) / d64).max()))
        for t in (0.01, 0.015, 0.02):
            near += int((np.abs(d64 - t) <= 1e-6 * t).sum())
    n = len(inp["pred"])
    dt = np.uint16 if n <= 65535 else np.int32
    out.update(comp_dist=comp.astype(np.float32), comp_idx=np.asarray(ci).astype(dt), comp_dot=comp_dot.astype(np.float32),
               acc_dist=acc.astype(np.float32), acc_idx=np.asarray(ai).astype(dt), acc_dot=acc_dot.astype(np.float32),
               near_tie_share=np.float64(share), near_threshold=np.int64(near), kdtree_vs_float64=np.float64(worst))
    assert comp.dtype == np.float32 and acc.dtype == np.float32
    metrics = ref_eval.MeshEvaluator().eval_pointcloud(inp["pred"], inp["tgt"], inp["n_pred"], inp["n_tgt"])
    keys = sorted(metrics)
    out["metric_keys"] = np.array(keys)
    out["metrics"] = np.array([float(metrics[k]) for k in keys], np.float64)
    t0 = time.perf_counter()
    c512 = ref_eval.check_mesh_contains(mesh, inp["pts"])
    out["contains_reference_seconds"] = np.float64(time.perf_counter() - t0)
    c128 = ref_eval.check_mesh_contains(mesh, inp["pts"], hash_resolution=128)
    assert np.array_equal(c512, eval_emu.mesh_contains(inp["v"], inp["f"], inp["pts"], 512))
    assert np.array_equal(c128, eval_emu.mesh_contains(inp["v"], inp["f"], inp["pts"], 128))
    out["contains_512"], out["contains_128"] = np.packbits(c512), np.packbits(c128)
    out["iou"] = np.float64(ref_eval.compute_iou(c512, inp["occ_tgt"]))
    print(name, "seed", seed, "N", n, "near-tie share", share, "points near a threshold", near, "KD-tree vs float64 %.3g" % worst,
          "inside", int(c512.sum()), int(c128.sum()), "iou %.6f" % float(out["iou"]),
          "reference seconds: nn %.3f contains %.3f" % (float(out["nn_reference_seconds"]), float(out["contains_reference_seconds"])))
    return out, share, near / (2.0 * n)


def main():
    g16 = np.load(os.path.join(ROOT, "tests", "golden", "g16_mesh.npz"))
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        ref_eval = reference_eval(tmp)
        for key, val in (("empty_pcl_keys", ref_eval.EMPTY_PCL_DICT), ("empty_normals_keys", ref_eval.EMPTY_PCL_DICT_NORMALS)):
            keys = sorted(val)
            out[key] = np.array(keys)
            out[key.replace("_keys", "_values")] = np.array([float(val[k]) for k in keys], np.float64)
        for name in eval_emu.CASES:
            for seed in range(0, 30, 3):
                case, tie_share, thr_share = run_case(ref_eval, g16, name, seed)
                if tie_share <= 1e-3 and thr_share <= 1e-3:
                    break
            else:
                raise SystemExit("no seed keeps the near-tie shares of case %s within 0.1 %%" % name)
            out.update({name + "_" + k: v for k, v in case.items()})
    path = os.path.join(ROOT, "tests", "golden", "g17_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 500_000


if __name__ == "__main__":
    t0 = time.time()
    main()
    print("%.1f s" % (time.time() - t0))
