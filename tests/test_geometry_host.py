"""CPU tests of the geometry scoring (giga_amd.geometry): the restatement of tests/geometry_emu.py against the live reference
data set, the point counts, the mesh files, the score formulas, the mean filter, the command line and the C ABI."""
import json
import os
import re
import sys

import numpy as np
import pytest

from giga_amd import _capi, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_emu as G  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------ the reference pin
@pytest.mark.reference
def test_roi_restatement_against_the_live_reference(tmp_path, monkeypatch):
    """DatasetVoxelOccGeoROI.__getitem__ on a synthetic set, its uniforms from a seeded generator: geometry_emu reproduces the
    world points (what check_occ receives) and the normalised points bit for bit, and both scene lists in order."""
    from oracle import ref_bootstrap
    if not ref_bootstrap.reference_available():
        pytest.skip("reference checkout not present")
    from pathlib import Path
    ref_bootstrap.install()
    import vgn.utils.implicit as implicit
    if not hasattr(implicit, "check_mesh_contains"):          # (libmesh is not built: the import inside the module failed)
        implicit.check_mesh_contains = lambda mesh, points: np.zeros(len(points), bool)
    from vgn.dataset_voxel_occ import DatasetVoxelOccGeo, DatasetVoxelOccGeoROI

    root, raw = tmp_path / "set", tmp_path / "raw"
    synth.write_training_set(str(root), str(raw), n_scenes=6, grasps_per_scene=5, seed=0)
    n = 257
    ds = DatasetVoxelOccGeoROI(Path(root), Path(raw), num_point_occ=n)
    seen = []
    ds.check_occ = lambda scene_id, points: (seen.append(points.copy()) or np.zeros(len(points), bool), None)
    ds.sample_occ = lambda scene_id, num: (np.zeros((num, 3), np.float32), np.zeros(num, bool), None)

    df, everything, positives = G.scene_lists(raw)
    assert DatasetVoxelOccGeo(Path(root), Path(raw)).scene_list == everything and len(everything) == 6
    assert ds.scene_list == list(positives)
    with open(raw / "setup.json") as f:
        setup = json.load(f)
    for i, sid in enumerate(ds.scene_list):
        rng, drawn = np.random.default_rng([5, i]), []

        def rand(*shape):
            u = rng.random(shape)
            drawn.append(u)
            return u.copy()                               # (the class changes the array in place)

        monkeypatch.setattr(np.random, "rand", rand)
        item = ds[i]
        monkeypatch.undo()
        R, pos, width = G.roi_grasps(df, positives[sid], setup["finger_depth"])
        assert 2 <= len(width) <= 4
        counts = G.point_counts(width, n)
        assert [len(u) for u in drawn] == list(counts)
        world, norm = G.roi_scene(R, pos, width, counts, np.concatenate(drawn), setup["finger_depth"], ds.ROI_scale, setup["size"],
                                  blas=True)
        assert world.dtype == seen[i].dtype == np.float64 and world.tobytes() == seen[i].tobytes()
        ref_norm = np.asarray(item[3])
        assert norm.tobytes() == ref_norm.astype(np.float32).tobytes()
        # the kernel's documented order differs from the matrix product by rounding only
        world2, _ = G.roi_scene(R, pos, width, counts, np.concatenate(drawn), setup["finger_depth"], ds.ROI_scale, setup["size"])
        assert np.abs(world2 - world).max() <= 1e-15


# ------------------------------------------------------------------------------------------------------------------ host pieces
def test_scene_lists_follow_first_appearance_and_drop_scenes_without_success(tmp_path):
    from giga_amd.geometry import VoxelOccGeoDataset, VoxelOccGeoROIDataset
    raw = tmp_path / "raw"
    raw.mkdir()
    rows = [("c", 0), ("a", 0), ("b", 1), ("a", 1), ("c", 0), ("d", 0), ("b", 0), ("e", 1)]
    with open(raw / "grasps.csv", "w") as f:
        f.write("scene_id,qx,qy,qz,qw,x,y,z,width,label\n")
        for k, (sid, label) in enumerate(rows):
            f.write("%s,0.0,0.0,0.0,1.0,0.1,0.1,0.1,%r,%d\n" % (sid, 0.04 + 0.01 * k, label))
    with open(raw / "setup.json", "w") as f:
        json.dump({"size": 0.3, "finger_depth": 0.05}, f)
    assert VoxelOccGeoDataset(tmp_path, raw).scene_list == ["c", "a", "b", "d", "e"]
    ds = VoxelOccGeoROIDataset(tmp_path, raw)
    assert ds.scene_list == ["a", "b", "e"] and len(ds) == 3
    df, everything, positives = G.scene_lists(raw)
    assert everything == ["c", "a", "b", "d", "e"] and list(positives) == ds.scene_list
    R, pos, width = ds.roi_grasps(1)
    eR, epos, ewidth = G.roi_grasps(df, positives["b"], 0.05)
    assert R.tobytes() == eR.tobytes() and pos.tobytes() == epos.tobytes() and width.tobytes() == ewidth.tobytes()
    assert width.tolist() == [0.06] and np.allclose(pos, [[0.1, 0.1, 0.15]])


def test_roi_point_counts_round_half_to_even():
    from giga_amd.geometry import roi_point_counts
    assert roi_point_counts([1.0, 1.0, 1.0], 256).tolist() == [85, 85, 85]                 # 85.33: the total is 255
    assert roi_point_counts([1.0, 1.0, 1.0], 2048).tolist() == [683, 683, 683]             # 682.67: the total is 2049
    assert roi_point_counts([1.0, 3.0], 10).tolist() == [2, 8]                             # 2.5 -> 2, 7.5 -> 8: half to even
    assert roi_point_counts([1.0, 1.0], 5).tolist() == [2, 2] and roi_point_counts([1.0, 1.0], 7).tolist() == [4, 4]
    assert roi_point_counts([1e-6, 0.08], 2048).tolist() == [0, 2048]                      # a very narrow grasp gets nothing
    w = [0.021, 0.08, 0.055, 0.034]
    assert roi_point_counts(w, 257).tolist() == G.point_counts(w, 257).tolist()
    assert roi_point_counts(w, 257).dtype.kind == "i"


def test_load_obj_quads_slashes_and_negative_indices(tmp_path):
    from giga_amd.geometry import default_mesh_loader, load_obj
    v, f = G.unit_box()
    G.write_obj(tmp_path / "quad.obj", v, f, quads=True)
    qv, qf = load_obj(tmp_path / "quad.obj")
    assert qv.dtype == np.float64 and qf.dtype == np.int64 and np.array_equal(qv, v) and qf.shape == (12, 3)
    assert qf[0].tolist() == [0, 3, 2] and qf[1].tolist() == [0, 2, 1]                     # a fan about the first corner
    assert qf[-2].tolist() == [0, 4, 7] and qf[-1].tolist() == [0, 7, 3]                   # -8//1 -4//1 -1//1 -5//1
    # the same closed surface: every edge is used twice, the volume is 1
    tri = qv[qf]
    vol = np.abs(np.einsum("ij,ij->i", tri[:, 0], np.cross(tri[:, 1], tri[:, 2])).sum()) / 6
    edges = np.sort(np.concatenate([qf[:, [0, 1]], qf[:, [1, 2]], qf[:, [2, 0]]]), axis=1)
    assert abs(vol - 1.0) < 1e-12 and (np.unique(edges, axis=0, return_counts=True)[1] == 2).all()
    with open(tmp_path / "mixed.obj", "w") as fh:
        fh.write("o thing\nv 0 0 0\nv 1 0 0\nvt 0 0\nv 0 1 0\nvn 0 0 1\nf 1/1 2/1 3/1\nv 0 0 1\nf -1 -2 -4\n\ns off\n")
    mv, mf = default_mesh_loader(str(tmp_path / "mixed.obj"))
    assert mv.shape == (4, 3) and mf.tolist() == [[0, 1, 2], [3, 2, 0]]
    with open(tmp_path / "bad.obj", "w") as fh:
        fh.write("v 0 0 0\nf 1 2 3\n")
    with pytest.raises(ValueError):
        load_obj(tmp_path / "bad.obj")


def test_urdf_loader_and_its_refusals(tmp_path):
    from giga_amd.geometry import default_mesh_loader
    v, f = G.unit_box()
    G.write_obj(tmp_path / "box.obj", v, f)

    def urdf(name, body):
        with open(tmp_path / name, "w") as fh:
            fh.write('<?xml version="1.0"?>\n<robot name="r">' + body + "</robot>\n")
        return str(tmp_path / name)

    visual = '<visual><geometry><mesh filename="box.obj"%s/></geometry></visual>'
    lv, lf = default_mesh_loader(urdf("ok.urdf", '<link name="a">' + visual % "" + "</link>"))
    assert np.array_equal(lv, v) and np.array_equal(lf, f)
    default_mesh_loader(urdf("ones.urdf", '<link name="a">' + visual % ' scale="1 1 1.0"' + "</link>"))
    with pytest.raises(NotImplementedError):
        default_mesh_loader(urdf("scaled.urdf", '<link name="a">' + visual % ' scale="1 1 2"' + "</link>"))
    with pytest.raises(ValueError):
        default_mesh_loader(urdf("links.urdf", '<link name="a">' + visual % "" + '</link><link name="b"/>'))
    with pytest.raises(ValueError):
        default_mesh_loader(urdf("visuals.urdf", '<link name="a">' + visual % "" + visual % "" + "</link>"))
    with pytest.raises(ValueError):
        default_mesh_loader(urdf("nomesh.urdf", '<link name="a"><visual><geometry><box size="1 1 1"/></geometry></visual></link>'))
    with pytest.raises(NotImplementedError):
        default_mesh_loader(str(tmp_path / "thing.stl"))


def test_read_mesh_pose_list_applies_scale_and_pose(tmp_path):
    from giga_amd import render
    from giga_amd.geometry import read_mesh_pose_list
    v, f = G.unit_box()
    G.write_obj(tmp_path / "box.obj", v, f)
    (tmp_path / "mesh_pose_list").mkdir()
    pose = np.eye(4)
    pose[:3, 3] = [0.1, 0.2, 0.05]
    pc = np.empty(2, dtype=object)
    pc[0] = (str(tmp_path / "box.obj"), np.array([0.06, 0.08, 0.1]), pose)
    pc[1] = (str(tmp_path / "box.obj"), 0.05, np.eye(4))
    np.savez(tmp_path / "mesh_pose_list" / "s.npz", pc=pc)
    mesh_pose_list, mesh_list = read_mesh_pose_list(tmp_path, "s")
    assert len(mesh_pose_list) == len(mesh_list) == 2
    sv, sf = render.scene_mesh(mesh_pose_list)
    assert sv.dtype == np.float32 and sv.shape == (16, 3) and sf.max() == 15
    assert np.array_equal(mesh_list[0][0], (v * [0.06, 0.08, 0.1] + [0.1, 0.2, 0.05]).astype(np.float32))
    assert np.array_equal(mesh_list[1][0], (v * 0.05).astype(np.float32)) and np.array_equal(mesh_list[1][1], f)
    assert np.array_equal(sv, np.concatenate([mesh_list[0][0], mesh_list[1][0]]))


def test_occ_scores_are_the_reference_formulas():
    from giga_amd.geometry import occ_scores
    rng = np.random.default_rng(3)
    cases = [(rng.random(1000) < 0.3, rng.random(1000) < 0.4), (np.zeros(50, bool), rng.random(50) < 0.5),
             (rng.random(50) < 0.5, np.zeros(50, bool)), (np.zeros(7, bool), np.zeros(7, bool)), (np.ones(9, bool), np.ones(9, bool)),
             (rng.random(100000) < 0.01, rng.random(100000) < 0.9)]
    for pred, occ in cases:
        got, want = occ_scores(G.confusion(pred, occ), "_ROI"), G.reference_scores(pred, occ, "_ROI")
        assert set(got) == set(want) == {"iou_ROI", "precision_ROI", "recall_ROI"}
        for k in want:
            assert G.same_number(got[k], want[k]), (k, got[k], want[k])
    z = occ_scores([0, 0, 0, 7])
    assert np.isnan(z["iou"]) and np.isnan(z["precision"]) and np.isnan(z["recall"]) and z["iou"].dtype == np.float32
    assert G.confusion(*cases[0]).sum() == 1000


def test_mean_filter_drops_nan_and_empty_scenes():
    from giga_amd.geometry import MEAN_KEYS, ROI_KEYS, mean_results
    assert MEAN_KEYS == ("iou", "chamfer-L1", "normals accuracy", "f-score")
    assert set(ROI_KEYS) == {n + e for n in ("iou", "precision", "recall") for e in ("_ROI", "_ROI_infer")}
    a = {"iou": 0.5, "chamfer-L1": 0.25, "normals accuracy": 0.75, "f-score": float("nan"), "completeness": 1.0}
    b = {"iou": np.float32(0.25), "chamfer-L1": 0.75, "normals accuracy": -1.0, "f-score": 0.5}
    e = {"iou": 0.0, "chamfer-L1": 6, "normals accuracy": -1.0, "empty": True}
    mean = mean_results([a, e, b], MEAN_KEYS, "some/model.pt")
    assert mean == {"model_path": os.path.abspath("some/model.pt"), "iou": 0.375, "chamfer-L1": 0.5, "normals accuracy": -0.125,
                    "f-score": 0.5}
    assert list(mean) == ["model_path"] + list(MEAN_KEYS) and all(type(mean[k]) is float for k in MEAN_KEYS)
    only_empty = mean_results([e], MEAN_KEYS)
    assert only_empty["model_path"] is None and all(np.isnan(only_empty[k]) for k in MEAN_KEYS)
    huge = dict(a, **{"f-score": -2e5})
    assert mean_results([huge, b], MEAN_KEYS)["f-score"] == 0.5            # the reference's own bound: >= -1e5


def test_parser_accepts_the_reference_command_line():
    from pathlib import Path
    from giga_amd import eval_geometry
    args = eval_geometry.build_parser().parse_args(
        ["--model-path", "m/vgn_giga_geo_10.pt", "--type", "giga_geo", "--dataset", "data/set", "--dataset_raw", "data/raw",
         "--logdir", "out", "--description", "run", "--ROI", "--th", "0.4", "--seed", "3"])
    assert args.model_path == "m/vgn_giga_geo_10.pt" and args.type == "giga_geo" and args.dataset == Path("data/set")
    assert args.dataset_raw == Path("data/raw") and args.logdir == Path("out") and args.description == "run" and args.ROI
    assert args.th == 0.4 and args.seed == 3
    assert (args.batch, args.precision, args.num_point_occ, args.n_points) == (8, "fp32", 100000, 100000)
    d = eval_geometry.build_parser().parse_args(["--dataset", "a", "--dataset_raw", "b"])
    assert d.logdir == Path("data/eval_geo") and d.description == "" and not d.ROI and d.th == 0.5 and d.seed == 42
    more = eval_geometry.build_parser().parse_args(["--dataset", "a", "--dataset_raw", "b", "--batch", "2", "--precision", "fp16x3",
                                                    "--num-point-occ", "2048", "--n-points", "2000"])
    assert (more.batch, more.precision, more.num_point_occ, more.n_points) == (2, "fp16x3", 2048, 2000)
    import datetime
    name = eval_geometry.run_directory(args, datetime.datetime(2024, 1, 2, 3, 4)).name
    assert name == "24-01-02-03-04_eval_geo_dataset=set,net=giga_geo,th=0.4,run"
    with pytest.raises(SystemExit):
        eval_geometry.build_parser().parse_args(["--dataset", "a"])


def test_new_symbols_are_declared_exported_and_additive():
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    lib = _capi.lib()
    for name in ("giga_roi_points", "giga_roi_points_workspace_bytes", "giga_occ_confusion", "giga_occ_confusion_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in _capi.EXPORTS and hasattr(lib, name)
    assert lib.giga_abi_version() == 3 and "#define GIGA_ABI_VERSION 3" in hdr
    assert "giga_geometry.o" in open(os.path.join(ROOT, "giga_amd", "csrc", "Makefile")).read()
    # argument checks that need no device: they answer before the first HIP call
    assert lib.giga_roi_points_workspace_bytes(0) == 0 and lib.giga_roi_points_workspace_bytes(3) >= 3 * 13 * 8 + 10 * 4
    assert lib.giga_occ_confusion_workspace_bytes(0) == 0 and lib.giga_occ_confusion_workspace_bytes(_capi.MAX_SCENES + 1) == 0
    offs = np.array([0, 4], np.int32)
    p = offs.ctypes.data
    assert lib.giga_occ_confusion(None, None, 0.0, None, p, -1, None, None, 0, None) == -1
    assert lib.giga_occ_confusion(None, None, 0.0, None, p, _capi.MAX_SCENES + 1, None, None, 0, None) == -7
    assert lib.giga_occ_confusion(None, None, 0.0, None, p, 0, None, None, 0, None) == 0
    assert lib.giga_occ_confusion(p, p, 0.0, p, p, 1, p, p, 1 << 20, None) == -1                  # both forms of the prediction
    assert lib.giga_occ_confusion(None, None, 0.0, p, p, 1, p, p, 1 << 20, None) == -1            # neither
    assert lib.giga_occ_confusion(p, None, float("nan"), p, p, 1, p, p, 1 << 20, None) == -1
    assert lib.giga_occ_confusion(p, None, 0.0, p, p, 1, None, p, 1 << 20, None) == -6
    assert lib.giga_occ_confusion(p, None, 0.0, p, p, 1, p, p, 1, None) == -4
    bad = np.array([1, 4], np.int32)
    assert lib.giga_occ_confusion(p, None, 0.0, p, bad.ctypes.data, 1, p, p, 1 << 20, None) == -1
    g, nan_g = np.zeros((1, 13)), np.full((1, 13), np.nan)
    ints, minus = np.zeros(1, np.int32), np.array([-1], np.int32)
    args = lambda **k: [k.get("g", g.ctypes.data), k.get("offs", p), k.get("scene", ints.ctypes.data), ints.ctypes.data,  # noqa: E731
                        k.get("G", 1), 0, 0.05, 0.3, k.get("size", 0.3), k.get("world", p), p, p, k.get("ws", 1 << 20), None]
    assert lib.giga_roi_points(*args(G=-1)) == -1 and lib.giga_roi_points(*args(G=0)) == 0
    assert lib.giga_roi_points(*args(size=0.0)) == -1 and lib.giga_roi_points(*args(size=float("inf"))) == -1
    assert lib.giga_roi_points(*args(offs=bad.ctypes.data)) == -1 and lib.giga_roi_points(*args(g=None)) == -1
    assert lib.giga_roi_points(*args(scene=minus.ctypes.data)) == -1
    assert lib.giga_roi_points(*args(g=nan_g.ctypes.data)) == -1
    assert lib.giga_roi_points(*args(world=None)) == -6 and lib.giga_roi_points(*args(ws=8)) == -4


def test_package_exports_the_geometry_names():
    import giga_amd
    from giga_amd import geometry
    for name in ("GeometryEvaluator", "VoxelOccGeoDataset", "VoxelOccGeoROIDataset", "occ_confusion", "occ_scores", "roi_point_counts",
                 "load_obj", "default_mesh_loader", "read_mesh_pose_list"):
        assert getattr(giga_amd, name) is getattr(geometry, name)
