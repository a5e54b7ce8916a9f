"""Scoring predicted geometry on the device: the reference's scripts/eval_geometry_voxel.py and the two data sets of
src/vgn/dataset_voxel_occ.py (`DatasetVoxelOccGeo`, `DatasetVoxelOccGeoROI`): scene IoU, chamfer-L1, normal consistency,
F-score, and occupancy IoU / precision / recall inside the region of interest (ROI) of the successful grasps.

    ds = VoxelOccGeoROIDataset(root, raw_root, num_point_occ=100000)
    per_scene, mean = GeometryEvaluator(net, threshold=0.5).evaluate(ds, roi=True, logdir="data/eval_geo/run")

The pieces are the package's own (`Generator3D`, `MeshEvaluator.eval_meshes`, `render.sample_iou_points`, `render.scene_mesh`,
`eval.sample_surface_batch`, `decode_occ`); new here are the mesh files (`load_obj`, a one-link URDF reader), the ROI point sampler
(`giga_roi_points`) and the occupancy score that stays on the device (`giga_occ_confusion`), both in csrc/giga_geometry.hip.
There is no CPU path.

Differences from the reference, all deliberate:
  * every random draw is counter based or seeded per scene -- the ROI points from Philox-4x32-10 keyed by (seed, data-set scene
    index, point index), the occupancy points from a device generator seeded from (seed, scene index), the ground-truth surface
    samples from the sampler of `giga_amd.eval` keyed by (seed, scene index) -- so a scene's numbers do not depend on the batch
    size or on what was scored before it (the reference draws everything from numpy's global generator);
  * "predicted occupied" from logits is `float64(logit) > log(th / (1 - th))`, not `float32 sigmoid(logit) > th`: the two differ
    only for logits within float32 rounding of the boundary (include/giga_hip.h, giga_occ_confusion);
  * occupancy points are normalised in float64 and rounded to float32 once;
  * meshes are written as binary `.ply` (`giga_amd.visual`'s writer), not `.glb`;
  * a URDF whose mesh element carries a `scale` other than ones raises NotImplementedError; meshes are read from `.obj` files.
"""
import json
import os
import xml.etree.ElementTree as ET
from collections import OrderedDict
from pathlib import Path

import numpy as np
import torch

from . import _capi, ragged, render
from .dataset import read_voxel_grid
from .eval import MeshEvaluator, mesh_contains_batch, sample_surface_batch
from .generation import Generator3D

MEAN_KEYS = ("iou", "chamfer-L1", "normals accuracy", "f-score")          # eval_geometry_voxel.py:45-51
ROI_KEYS = tuple(name + ext for name in ("iou", "precision", "recall") for ext in ("_ROI", "_ROI_infer"))     # :52-55


# ------------------------------------------------------------------------------------------------------------------ mesh files
def load_obj(path):
    """Wavefront .obj -> (vertices (V,3) float64, faces (F,3) int64): `v x y z` and `f` lines with the `a`, `a/b`, `a//c`, `a/b/c`
    forms, negative (relative) indices, polygons fan-triangulated about their first corner.  Everything else is skipped."""
    vertices, faces = [], []
    with open(path, "r") as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if parts[0] == "v":
                vertices.append([float(x) for x in parts[1:4]])
            elif parts[0] == "f":
                idx = []
                for corner in parts[1:]:
                    k = int(corner.split("/")[0])
                    k = k - 1 if k > 0 else len(vertices) + k
                    if k < 0 or k >= len(vertices):
                        raise ValueError(f"{path}: face index {corner!r} outside the vertices read so far")
                    idx.append(k)
                for j in range(1, len(idx) - 1):
                    faces.append([idx[0], idx[j], idx[j + 1]])
    return np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3)


def _urdf_mesh_path(path):
    """utils/implicit.py:58-63: exactly one link, one visual, one mesh"""
    root = ET.parse(path).getroot()
    links = root.findall("link")
    if len(links) != 1:
        raise ValueError(f"{path}: expected one link, found {len(links)}")
    visuals = links[0].findall("visual")
    if len(visuals) != 1:
        raise ValueError(f"{path}: expected one visual, found {len(visuals)}")
    meshes = visuals[0].findall("geometry/mesh")
    if len(meshes) != 1:
        raise ValueError(f"{path}: expected one mesh, found {len(meshes)}")
    scale = meshes[0].get("scale")
    if scale is not None and [float(s) for s in scale.split()] != [1.0, 1.0, 1.0]:
        raise NotImplementedError(f"{path}: a mesh scale other than ones is not built")
    name = meshes[0].get("filename")
    if not name:
        raise ValueError(f"{path}: the mesh has no filename")
    if name.startswith("package://"):
        name = name[len("package://"):]
    return name if os.path.isabs(name) else os.path.join(os.path.dirname(str(path)), name)


def default_mesh_loader(path):
    """`.obj`, or a `.urdf` with one link, one visual and one `.obj` mesh -> (vertices float64, faces int64)"""
    path = str(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".urdf":
        path = _urdf_mesh_path(path)
        ext = os.path.splitext(path)[1].lower()
    if ext != ".obj":
        raise NotImplementedError(f"{path}: only .obj meshes are read (pass a mesh_loader for other formats)")
    return load_obj(path)


def read_mesh_pose_list(raw_root, scene_id, mesh_loader=None):
    """<raw_root>/mesh_pose_list/<scene_id>.npz, key `pc`: an object array of (mesh_path, scale, pose 4x4).  Returns
    (mesh_pose_list, mesh_list): the [(vertices, faces, scale, pose)] list `render.scene_mesh` takes, and per object the
    (vertices float32, faces int32) mesh with scale and pose applied (the reference's `mesh_list`)."""
    loader = mesh_loader if mesh_loader is not None else default_mesh_loader
    pc = np.load(Path(raw_root) / "mesh_pose_list" / (str(scene_id) + ".npz"), allow_pickle=True)["pc"]
    mesh_pose_list = []
    for mesh_path, scale, pose in pc:
        v, f = loader(str(mesh_path))
        mesh_pose_list.append((v, f, scale, pose))
    return mesh_pose_list, [render.scene_mesh([entry]) for entry in mesh_pose_list]


# -------------------------------------------------------------------------------------------------------------------- data sets
def _scene_seed(seed, i):
    return int(np.random.SeedSequence([int(seed), int(i)]).generate_state(1, np.uint64)[0] & np.uint64(2 ** 63 - 1))


class VoxelOccGeoDataset:
    """`DatasetVoxelOccGeo` (dataset_voxel_occ.py:12-52): one item per scene of grasps.csv, in order of first appearance."""

    uniform, padding = False, 0.02             # sample_iou_points' defaults (utils/implicit.py:78)

    def __init__(self, root, raw_root, num_point_occ=2048, mesh_loader=None, seed=0, device=None):
        import pandas as pd
        self.root, self.raw_root = Path(root), Path(raw_root)
        self.num_point_occ = int(num_point_occ)
        self.mesh_loader = mesh_loader
        self.seed = int(seed)
        self.device = device
        self.df = pd.read_csv(self.raw_root / "grasps.csv")                   # io.py:80-81
        with (self.raw_root / "setup.json").open("r") as f:                   # io.py:19-26
            setup = json.load(f)
        self.size, self.finger_depth = setup["size"], setup.get("finger_depth")
        self.scene_list = self._scene_list()

    def _scene_list(self):
        return list(OrderedDict.fromkeys(self.df["scene_id"].astype(str).tolist()))

    def __len__(self):
        return len(self.scene_list)

    def scene(self, i):
        """(grid (40,40,40) float32, scene mesh (vertices float32, faces int32) in world coordinates, mesh list)"""
        scene_id = self.scene_list[i]
        grid = read_voxel_grid(self.root, scene_id)[0]
        mesh_pose_list, mesh_list = read_mesh_pose_list(self.raw_root, scene_id, self.mesh_loader)
        return grid, render.scene_mesh(mesh_pose_list), mesh_list

    def _occ(self, i, mesh_list):
        """dataset_voxel_occ.py:35-36, 40-45: (points (n,3) float32 normalised, occ (n,) bool) on the device"""
        dev = _capi.hip_device(device=self.device, what="geometry scoring runs only on a HIP device")
        gen = torch.Generator(device=dev)
        gen.manual_seed(_scene_seed(self.seed, i))
        kwargs = dict(uniform=True, size=self.size, padding=0) if self.uniform else dict(uniform=False, padding=self.padding)
        points, occ = render.sample_iou_points(mesh_list, render.mesh_bounds(mesh_list), self.num_point_occ, generator=gen,
                                               device=dev, **kwargs)
        return (points.double() / self.size - 0.5).float(), occ

    def item(self, i):
        return self.items([i])[0]

    def items(self, indices):
        """one dict per scene: grid, points, occ, scene_mesh, mesh_list"""
        out = []
        for i in indices:
            grid, scene, mesh_list = self.scene(i)
            points, occ = self._occ(i, mesh_list)
            out.append(dict(grid=grid, points=points, occ=occ, scene_mesh=scene, mesh_list=mesh_list))
        return out


def roi_point_counts(widths, n):
    """dataset_voxel_occ.py:110-113: points per grasp in proportion to its width, numpy's round (half to even).  The sum need
    not be n."""
    num = n * np.array(widths, dtype=float)
    num /= np.sum(np.array(widths, dtype=float))
    return np.round(num).astype(int)


def roi_points(grasps, counts, scenes, seed, finger_depth, ROI_scale, size, device=None):
    """dataset_voxel_occ.py:115-128 for a ragged batch of scenes in one `giga_roi_points` launch.  Per scene: grasps = (R (k,3,3),
    pos (k,3), width (k,)) float64, counts = (k,) points per grasp, scenes = its index in the data set (the generator's scene
    word).  Returns (world (n,3) float64, normalised (n,3) float32 = float32(world / size - 0.5), scene offsets (len + 1) int32 on
    the host); a scene's rows list its grasps in order."""
    dev = _capi.hip_device(device=device, what="the ROI points are drawn on a HIP device")
    table, scene, first, per_scene = [], [], [], []
    for (R, pos, width), cnt, i in zip(grasps, counts, scenes):
        cnt = np.asarray(cnt, np.int64).reshape(-1)
        R, pos, width = np.asarray(R, np.float64), np.asarray(pos, np.float64), np.asarray(width, np.float64)
        if not (len(R) == len(pos) == len(width) == len(cnt)) or (cnt < 0).any():
            raise ValueError("one rotation, position, width and non-negative count per grasp")
        table.append(np.concatenate((R.reshape(-1, 9), pos.reshape(-1, 3), width.reshape(-1, 1)), axis=1))
        scene.append(np.full(len(cnt), int(i), np.int64))
        first.append(np.cumsum(cnt) - cnt)
        per_scene.append(int(cnt.sum()))
    scene_offsets = ragged.offsets(per_scene)
    n = int(scene_offsets[-1])
    world = torch.empty((n, 3), dtype=torch.float64, device=dev)
    normalised = torch.empty((n, 3), dtype=torch.float32, device=dev)
    if n:
        table = np.ascontiguousarray(np.concatenate(table), np.float64)
        offs = ragged.offsets(np.concatenate([np.asarray(c, np.int64).reshape(-1) for c in counts]))
        scene = np.ascontiguousarray(np.concatenate(scene), np.int32)
        first = np.ascontiguousarray(np.concatenate(first), np.int32)
        G = len(scene)
        ws = _capi.workspace("giga_roi_points", dev, G)
        _capi.call("giga_roi_points", dev, table, offs, scene, first, G, int(seed) & (2 ** 64 - 1), float(finger_depth),
                   float(ROI_scale), float(size), world, normalised, ws, ws.numel())
    return world, normalised, scene_offsets


class VoxelOccGeoROIDataset(VoxelOccGeoDataset):
    """`DatasetVoxelOccGeoROI` (dataset_voxel_occ.py:54-168): the scenes with at least one successful grasp; next to the
    uniform occupancy points, points inside a box at the finger tips of every successful grasp (`giga_roi_points`) with the union of
    `giga_mesh_contains` over the scene's objects as labels."""

    padding = 0

    def __init__(self, root, raw_root, num_point_occ=2048, ROI_scale=0.3, uniform=True, mesh_loader=None, seed=0, device=None):
        self.ROI_scale = ROI_scale
        self.uniform = uniform
        super().__init__(root, raw_root, num_point_occ, mesh_loader, seed, device)
        if self.finger_depth is None:
            raise ValueError("setup.json has no finger_depth")
        self._quat = self.df.loc[:, "qx":"qw"].to_numpy(np.single)            # :100-101
        self._xyz = self.df.loc[:, "x":"z"].to_numpy(np.float64)              # :102
        self._width = self.df["width"].to_numpy().astype(np.float64)          # :103

    def _scene_list(self):
        self.scene_dict = OrderedDict()
        for i, (scene_id, label) in enumerate(zip(self.df["scene_id"].astype(str).tolist(), self.df["label"].tolist())):
            rows = self.scene_dict.setdefault(scene_id, [])
            if label:
                rows.append(i)
        for k in [k for k, v in self.scene_dict.items() if len(v) < 1]:
            self.scene_dict.pop(k)
        return list(self.scene_dict.keys())

    def roi_grasps(self, i):
        """(R (k,3,3), pos (k,3), width (k,)) float64 of scene i's successful grasps: dataset_voxel_occ.py:99-107, on the host
        with scipy as the reference does (the quaternion read as float32; pos = xyz + R (0,0,1) finger_depth)"""
        from scipy.spatial.transform import Rotation
        rows = self.scene_dict[self.scene_list[i]]
        R, pos = np.empty((len(rows), 3, 3)), np.empty((len(rows), 3))
        for k, row in enumerate(rows):
            ori = Rotation.from_quat(self._quat[row])
            p = self._xyz[row].copy()
            p += ori.apply(np.array([0, 0, 1])) * self.finger_depth
            R[k], pos[k] = ori.as_matrix(), p
        return R, pos, self._width[rows].copy()

    def roi_points(self, indices):
        """ROI points of the scenes `indices` in one launch (module function `roi_points`): scene i's points are the same
        whatever else is in the call."""
        grasps = [self.roi_grasps(i) for i in indices]
        counts = [roi_point_counts(g[2], self.num_point_occ) for g in grasps]
        return roi_points(grasps, counts, indices, self.seed, self.finger_depth, self.ROI_scale, self.size, self.device)

    @staticmethod
    def roi_labels(world, scene_offsets, mesh_lists):
        """check_occ (dataset_voxel_occ.py:136-146) for all scenes: the union over every scene's objects of the containment of its
        float64 world points, one ragged launch -> (n,) bool on the device"""
        occ = torch.zeros(len(world), dtype=torch.bool, device=world.device)
        meshes, points, where = [], [], []
        for b, mesh_list in enumerate(mesh_lists):
            a, e = int(scene_offsets[b]), int(scene_offsets[b + 1])
            for m in mesh_list:
                if e > a and len(m[1]):
                    meshes.append(m)
                    points.append(world[a:e])
                    where.append((a, e))
        if meshes:
            inside, po = mesh_contains_batch(meshes, points)
            for k, (a, e) in enumerate(where):
                occ[a:e] |= inside[po[k]:po[k + 1]]
        return occ

    def items(self, indices):
        """VoxelOccGeoDataset.items plus roi_points (normalised float32), roi_world (float64) and roi_occ per scene"""
        out = super().items(indices)
        world, normalised, so = self.roi_points(indices)
        occ = self.roi_labels(world, so, [it["mesh_list"] for it in out])
        for b, it in enumerate(out):
            a, e = int(so[b]), int(so[b + 1])
            it.update(roi_points=normalised[a:e], roi_world=world[a:e], roi_occ=occ[a:e])
        return out


# ------------------------------------------------------------------------------------------------------------- occupancy scores
def logit_threshold(th):
    """log(th / (1 - th)) in float64: the right side of giga_occ_confusion's predicate"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.log(np.float64(th) / (np.float64(1.0) - np.float64(th))))


def occ_confusion(pred_or_logits, target, offsets, threshold=None):
    """Per-scene confusion counts of a ragged batch -> (B,4) int64 numpy [tp, fp, fn, tn], after ONE copy of 32 B bytes.
    target: (n,) bool / uint8 device tensor; offsets: (B+1) host prefix.  threshold None: pred_or_logits is (n,) bool / uint8;
    otherwise (n,) float32 logits and predicted = float64(logit) > log(threshold / (1 - threshold)) (NaN predicts false)."""
    dev = _capi.device_of(pred_or_logits, target)
    offs = np.ascontiguousarray(offsets, np.int32)
    B = len(offs) - 1
    if B < 0 or len(target.reshape(-1)) != int(offs[-1]) or len(pred_or_logits.reshape(-1)) != int(offs[-1]):
        raise ValueError("offsets do not cover the prediction and the target")

    def bytes_of(t):
        t = t.detach().reshape(-1).contiguous()
        return t.view(torch.uint8) if t.dtype == torch.bool else t.to(torch.uint8)

    tgt = bytes_of(target)
    if threshold is None:
        logits, pred, th = None, bytes_of(pred_or_logits), 0.0
    else:
        logits, pred, th = pred_or_logits.detach().reshape(-1).to(torch.float32).contiguous(), None, logit_threshold(threshold)
        if th != th:
            raise ValueError(f"threshold {threshold} has no logit")
    if B == 0:
        return np.zeros((0, 4), np.int64)
    counts = torch.empty((B, 4), dtype=torch.int64, device=dev)
    ws = _capi.workspace("giga_occ_confusion", dev, B)
    _capi.call("giga_occ_confusion", dev, logits, pred, th, tgt, offs, B, counts, ws, ws.numel())
    return counts.cpu().numpy()


def occ_scores(counts, ext=""):
    """[tp, fp, fn, tn] -> iou, precision, recall with the reference's formulas: iou as common.compute_iou gives it (float32
    intersection / float32 union), precision = tp / (tp + fp) and recall = tp / (tp + fn) in float64 (eval.py, eval_occ);
    0 / 0 gives NaN as numpy gives the reference.  (Exact below 2^24 points per scene, where float32 holds the counts.)"""
    tp, fp, fn = (np.int64(int(c)) for c in counts[:3])
    with np.errstate(invalid="ignore", divide="ignore"):
        return {"iou" + ext: np.float32(tp) / np.float32(tp + fp + fn),
                "precision" + ext: 1.0 * tp / (tp + fp),
                "recall" + ext: 1.0 * tp / (tp + fn)}


def mean_results(results, keys, model_path=None):
    """eval_geometry_voxel.py:45-55, 91-95, 104-107: the mean of every key over the scenes without `empty`, of the values
    >= -1e5 (which drops NaN); numpy's mean of nothing is NaN"""
    lists = {k: [] for k in keys}
    for out in results:
        if "empty" in out:
            continue
        for k in keys:
            if out[k] >= -1e5:
                lists[k].append(out[k])
    mean = {"model_path": os.path.abspath(model_path) if model_path is not None else None}
    with np.errstate(invalid="ignore"):
        for k in keys:
            mean[k] = float(np.mean(lists[k])) if lists[k] else float("nan")
    return mean


# ----------------------------------------------------------------------------------------------------------------- the driver
class GeometryEvaluator:
    """eval_geometry_voxel.py's main loop, `batch` scenes per encoder call."""

    def __init__(self, net, threshold=0.5, generator=None, n_points=100000, batch=8, seed=42, model_path=None):
        if int(batch) < 1:
            raise ValueError("batch must be at least 1")
        self.net = net
        self.threshold = threshold
        self.generator = generator if generator is not None else Generator3D(net, threshold=threshold, padding=0)
        self.n_points = int(n_points)
        self.batch = int(batch)
        self.seed = int(seed)
        self.model_path = model_path

    def evaluate(self, dataset, roi=False, logdir=None, export_meshes=False):
        """-> (one dict per scene, the dict of means).  With `roi` the data set is a VoxelOccGeoROIDataset and the scenes whose
        predicted mesh is not empty also get iou / precision / recall `_ROI` (the predicted mesh on the ROI points) and `_ROI_infer`
        (decode_occ on the planes of the same encoder call).  logdir: `%05d/results.json` per scene and `mean_results.json`;
        export_meshes: `gt_mesh.ply` / `pred_mesh.ply` (normalised coordinates) of the scenes that are not empty."""
        results = []
        if logdir is not None:
            Path(logdir).mkdir(parents=True, exist_ok=True)
        for at in range(0, len(dataset), self.batch):
            indices = list(range(at, min(at + self.batch, len(dataset))))
            outs, meshes, gts = self._score(dataset, indices, roi)
            for b, i in enumerate(indices):
                if logdir is not None:
                    save_dir = Path(logdir) / ("%05d" % i)
                    save_dir.mkdir(exist_ok=True)
                    if export_meshes and "empty" not in outs[b]:
                        _export_ply(save_dir / "gt_mesh.ply", *gts[b])
                        _export_ply(save_dir / "pred_mesh.ply", meshes[b].vertices, meshes[b].faces)
                    with open(save_dir / "results.json", "w") as f:
                        json.dump({k: float(v) for k, v in outs[b].items()}, f, indent=4)
            results += outs
        mean = mean_results(results, MEAN_KEYS + (ROI_KEYS if roi else ()), self.model_path)
        if logdir is not None:
            with open(Path(logdir) / "mean_results.json", "w") as f:
                json.dump(mean, f, indent=4)
        return results, mean

    def _score(self, dataset, indices, roi):
        items = dataset.items(indices)
        gen, B = self.generator, len(indices)
        dev = torch.device(gen.device)
        self.net.eval()
        c = gen.encode(torch.from_numpy(np.stack([np.asarray(it["grid"], np.float32) for it in items])))
        meshes = gen._meshes(gen.value_grid(c), c, {})
        # eval_geometry_voxel.py:79, 140-141: the ground truth in the model's coordinates, sampled with its face normals; scene i
        # draws with the generator's scene word i
        gts = [((np.asarray(it["scene_mesh"][0], np.float64) / dataset.size - 0.5).astype(np.float32), it["scene_mesh"][1]) for it in items]
        cloud, _, normal, counts = sample_surface_batch(gts, self.n_points, self.seed, indices[0])
        if int(counts.min()) == 0:
            raise ValueError("a ground-truth scene mesh has no surface to sample")
        outs = MeshEvaluator(self.n_points, self.seed).eval_meshes(meshes, list(cloud), list(normal), [it["points"] for it in items],
                                                                   [it["occ"] for it in items])
        live = [b for b in range(B) if "empty" not in outs[b]]
        if not live:
            return outs, meshes, gts
        # occupancy of the predicted meshes: one containment launch over the IoU points (and the ROI points) of every live scene,
        # one confusion launch; only the counts come back
        seg_mesh, seg_points, seg_target = [], [], []
        for b in live:
            for p, t in ((("points", "occ"),) + ((("roi_points", "roi_occ"),) if roi else ())):
                seg_mesh.append(meshes[b])
                seg_points.append(items[b][p])
                seg_target.append(items[b][t].reshape(-1))
        inside, po = mesh_contains_batch(seg_mesh, seg_points)
        counts = occ_confusion(inside, torch.cat(seg_target), po)
        step = 2 if roi else 1
        for k, b in enumerate(live):
            outs[b]["iou"] = occ_scores(counts[step * k])["iou"]
            if roi:
                outs[b].update(occ_scores(counts[step * k + 1], "_ROI"))
        if roi:
            # eval_points_infer (:152-162) on the cached planes: rows padded to the longest scene, the offsets skip the pads
            lens = [len(it["roi_points"]) for it in items]
            p = torch.zeros((B, max(max(lens), 1), 3), dtype=torch.float32, device=dev)
            for b, it in enumerate(items):
                p[b, :lens[b]] = it["roi_points"]
            with torch.no_grad():
                logits = self.net.decode_occ(p, c).logits
            packed = torch.cat([logits[b, :lens[b]] for b in live])
            counts = occ_confusion(packed, torch.cat([items[b]["roi_occ"] for b in live]), ragged.offsets([lens[b] for b in live]),
                                   threshold=self.threshold)
            for k, b in enumerate(live):
                outs[b].update(occ_scores(counts[k], "_ROI_infer"))
        return outs, meshes, gts


def _export_ply(path, vertices, faces):
    from .visual import ColoredMesh
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ColoredMesh(vertices, faces, np.full((len(faces), 4), 255, np.uint8)).export(str(path))
