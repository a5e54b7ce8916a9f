"""Mesh evaluation on the device, mirroring the reference's `vgn.ConvONets.eval` (eval.py:28-232): chamfer distances, F-score,
normal consistency and IoU of a predicted mesh against a target cloud, through the kernels of csrc/giga_eval.hip
(giga_nn_query, giga_mesh_sample, giga_mesh_contains).  A mesh is a `giga_amd.mesh.Mesh` or a `(vertices, faces)` pair of numpy
arrays or device tensors; point clouds are numpy arrays or device tensors.  There is no CPU path: numpy inputs are copied to the
current HIP device, CPU tensors raise `GigaHipError` like the other entry points.

Differences from the reference, all deliberate:
  * the surface sampler is this project's own counter-based one (`sample_surface`, Philox-4x32-10 keyed by seed, scene and sample
    index), not `trimesh.sample` on `np.random`;
  * `remove_wall=True` raises NotImplementedError (it needs a second random subsampling);
  * `eval_occ` on an empty mesh returns iou 0, precision NaN, recall NaN (the reference raises a NameError there).
"""
import logging

import numpy as np
import torch

from . import _capi, ragged

# Maximum values for the bounding box [-0.5, 0.5]^3
EMPTY_PCL_DICT = {
    'completeness': np.sqrt(3),
    'accuracy': np.sqrt(3),
    'completeness2': 3,
    'accuracy2': 3,
    'chamfer': 6,
    'empty': True,
}
EMPTY_PCL_DICT_NORMALS = {
    'normals completeness': -1.,
    'normals accuracy': -1.,
    'normals': -1.,
}
DEFAULT_THRESHOLDS = np.linspace(1. / 1000, 1, 1000)

logger = logging.getLogger(__name__)


# --------------------------------------------------------------------------------------------------------- the three kernels
def nn_query_batch(points_src, points_tgt):
    """lists of B source / target clouds -> (dist float32, idx int64 relative to the scene's targets, source offsets), packed"""
    dev = _capi.hip_device(*points_src, *points_tgt)
    src, so = ragged.pack(points_src, dev, torch.float32)
    tgt, to = ragged.pack(points_tgt, dev, torch.float32)
    B, n = len(so) - 1, int(so[-1])
    dist = torch.empty(n, dtype=torch.float32, device=dev)
    idx = torch.empty(n, dtype=torch.int32, device=dev)
    ws = _capi.workspace("giga_nn_query", dev, B, n)
    _capi.call("giga_nn_query", dev, src, so, tgt, to, B, dist, idx, ws, ws.numel())
    return dist, idx.to(torch.int64), so


def sample_surface_batch(meshes, n, seed=0, first_scene=0):
    """B meshes -> (points (B,n,3) float32, face (B,n) int64, normals (B,n,3) float32, counts (B,) int64 on the host); a scene
    whose count is 0 (no faces, no area) has zero rows.  Scene b draws with the generator's scene word first_scene + b"""
    dev = _capi.hip_device(*ragged.mesh_arrays(meshes))
    v, vo, f, fo = ragged.pack_meshes(meshes, dev)
    B = len(vo) - 1
    points = torch.zeros((B, n, 3), dtype=torch.float32, device=dev)
    face = torch.zeros((B, n), dtype=torch.int32, device=dev)
    normals = torch.zeros((B, n, 3), dtype=torch.float32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    ws = _capi.workspace("giga_mesh_sample", dev, B, int(fo[-1]))
    _capi.call("giga_mesh_sample", dev, v, vo, f, fo, B, int(n), int(seed) & (2 ** 64 - 1), int(first_scene), points, face, normals,
               counts, ws, ws.numel())
    return points, face.to(torch.int64), normals, counts.cpu().to(torch.int64)


def mesh_contains_batch(meshes, points, hash_resolution=512):
    """B meshes, B query clouds -> (inside bool, packed; point offsets)"""
    dev = _capi.hip_device(*ragged.mesh_arrays(meshes), *points)
    v, vo, f, fo = ragged.pack_meshes(meshes, dev)
    p, po = ragged.pack(points, dev, torch.float64)
    B, n = len(vo) - 1, int(po[-1])
    inside = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws = _capi.workspace("giga_mesh_contains", dev, B, int(fo[-1]), n)
    _capi.call("giga_mesh_contains", dev, v, vo, f, fo, p, po, B, int(hash_resolution), inside, ws, ws.numel())
    return inside.to(torch.bool), po


# ------------------------------------------------------------------------------------------- the reference's module functions
def sample_surface(mesh, n, seed=0, scene=0):
    """n points uniform over the mesh's surface -> (points (n,3) float32, face_index (n,) int64, normals (n,3) float32), device
    tensors; all three are empty for a mesh without faces or without area"""
    p, f, nr, counts = sample_surface_batch([mesh], n, seed, scene)
    k = int(counts[0])
    return p[0, :k], f[0, :k], nr[0, :k]


def check_mesh_contains(mesh, points, hash_resolution=512):
    """bool device tensor: which points lie inside the mesh (the reference's libmesh.check_mesh_contains)"""
    return mesh_contains_batch([mesh], [points], hash_resolution)[0]


def _normal_dots(idx, normals_src, normals_tgt, dev):
    ns, nt = ragged.to_device(normals_src, dev, torch.float32), ragged.to_device(normals_tgt, dev, torch.float32)
    ns = ns / ns.norm(dim=-1, keepdim=True)
    nt = nt / nt.norm(dim=-1, keepdim=True)
    return (nt[idx] * ns).sum(dim=-1).abs()


def distance_p2p(points_src, normals_src, points_tgt, normals_tgt):
    """minimal distance of every source point to the target points, and |n_tgt[nearest] . n_src| (NaN without normals)"""
    dist, idx, _ = nn_query_batch([points_src], [points_tgt])
    if normals_src is not None and normals_tgt is not None:
        dots = _normal_dots(idx, normals_src, normals_tgt, dist.device)
    else:
        dots = torch.full((len(dist),), float("nan"), dtype=torch.float32, device=dist.device)
    return dist, dots


def get_threshold_percentage(dist, thresholds):
    """share of distances <= t for every threshold: float32 distances against float64 thresholds, compared in float64"""
    d = (dist.detach() if torch.is_tensor(dist) else torch.from_numpy(np.ascontiguousarray(dist))).to(torch.float64).reshape(-1)
    t = torch.as_tensor(np.asarray(thresholds, np.float64), device=d.device)     # (plumbing: runs where the distances live)
    d, _ = torch.sort(d)
    below = torch.searchsorted(d, t, right=True)                  # number of d <= t
    return [float(x) for x in (below.to(torch.float64) / len(d)).cpu()]


def compute_iou(occ1, occ2):
    """the reference's common.compute_iou: >= 0.5, intersection / union (float32 like the reference's)"""
    a = occ1.detach().cpu().numpy() if torch.is_tensor(occ1) else np.asarray(occ1)
    b = occ2.detach().cpu().numpy() if torch.is_tensor(occ2) else np.asarray(occ2)
    if a.ndim >= 2:
        a = a.reshape(a.shape[0], -1)
    if b.ndim >= 2:
        b = b.reshape(b.shape[0], -1)
    a, b = a >= 0.5, b >= 0.5
    with np.errstate(invalid="ignore", divide="ignore"):
        return (a & b).astype(np.float32).sum(axis=-1) / (a | b).astype(np.float32).sum(axis=-1)


def _pointcloud_dict(comp, comp_dot, acc, acc_dot, thresholds):
    """eval.py:128-180 on device tensors; means accumulate in float64"""
    recall = get_threshold_percentage(comp, thresholds)
    precision = get_threshold_percentage(acc, thresholds)
    c64, a64 = comp.double(), acc.double()
    completeness, accuracy = float(c64.mean()), float(a64.mean())
    completeness2, accuracy2 = float((c64 * c64).mean()), float((a64 * a64).mean())
    cn, an = float(comp_dot.double().mean()), float(acc_dot.double().mean())
    with np.errstate(invalid="ignore", divide="ignore"):
        F = [2 * np.float64(precision[i]) * recall[i] / (np.float64(precision[i]) + recall[i]) for i in range(len(precision))]
    return {
        'completeness': completeness,
        'accuracy': accuracy,
        'normals completeness': cn,
        'normals accuracy': an,
        'normals': 0.5 * cn + 0.5 * an,
        'completeness2': completeness2,
        'accuracy2': accuracy2,
        'chamfer-L2': 0.5 * (completeness2 + accuracy2),
        'chamfer-L1': 0.5 * (completeness + accuracy),
        'f-score': F[9],        # threshold = 1.0%
        'f-score-15': F[14],    # threshold = 1.5%
        'f-score-20': F[19],    # threshold = 2.0%
    }


def _empty_dict(with_normals):
    logger.warning('Empty pointcloud / mesh detected!')
    out = EMPTY_PCL_DICT.copy()
    if with_normals:
        out.update(EMPTY_PCL_DICT_NORMALS)
    return out


def _is_empty(mesh):
    v, f = ragged.mesh_parts(mesh)
    return len(v) == 0 or len(f) == 0


class MeshEvaluator(object):
    """Mesh evaluation (the reference's class of the same name).  n_points: samples drawn on the predicted surface;
    seed: the sampler's seed."""

    def __init__(self, n_points=100000, seed=0):
        self.n_points = n_points
        self.seed = seed

    def eval_mesh(self, mesh, pointcloud_tgt, normals_tgt, points_iou, occ_tgt, remove_wall=False, seed=None):
        return self.eval_meshes([mesh], [pointcloud_tgt], [normals_tgt], [points_iou], [occ_tgt], remove_wall, seed)[0]

    def eval_meshes(self, meshes, pointclouds_tgt, normals_tgt, points_iou, occ_tgt, remove_wall=False, seed=None):
        """B scenes, one launch per stage; returns B dictionaries equal to B eval_mesh calls.  Every scene draws the samples a
        single call draws (the generator is keyed with scene 0 in both)."""
        if remove_wall:
            raise NotImplementedError("remove_wall needs a second random subsampling, which is not built")
        seed = self.seed if seed is None else seed
        B = len(meshes)
        if normals_tgt is None:
            normals_tgt = [None] * B
        live = [b for b in range(B) if not _is_empty(meshes[b])]
        clouds, normals = {}, {}
        for b in live:          # (one sampler call per scene keeps the key (seed, 0, i) of a single call)
            p, _, nr = sample_surface(meshes[b], self.n_points, seed)
            clouds[b], normals[b] = p, nr
        live = [b for b in live if len(clouds[b])]
        out = [None] * B
        for b in range(B):
            if b not in live:
                out[b] = _empty_dict(normals_tgt[b] is not None)
                out[b]['iou'] = 0.
        if live:
            dicts = self._eval_pointclouds([clouds[b] for b in live], [pointclouds_tgt[b] for b in live],
                                           [normals[b] for b in live], [normals_tgt[b] for b in live], DEFAULT_THRESHOLDS)
            occ, po = mesh_contains_batch([meshes[b] for b in live], [points_iou[b] for b in live])
            occ = occ.cpu().numpy()
            for k, b in enumerate(live):
                out[b] = dicts[k]
                out[b]['iou'] = compute_iou(occ[po[k]:po[k + 1]], occ_tgt[b])
        return out

    def eval_occ(self, mesh, points_iou, occ_tgt, ext=''):
        out_dict = {}
        occ_tgt = occ_tgt.detach().cpu().numpy() if torch.is_tensor(occ_tgt) else np.asarray(occ_tgt)
        if not _is_empty(mesh):
            occ = check_mesh_contains(mesh, points_iou).cpu().numpy()
            out_dict['iou' + ext] = compute_iou(occ, occ_tgt)
            with np.errstate(invalid="ignore", divide="ignore"):
                out_dict['precision' + ext] = 1.0 * np.sum(np.logical_and(occ, occ_tgt)) / np.sum(occ)
                out_dict['recall' + ext] = 1.0 * np.sum(np.logical_and(occ, occ_tgt)) / np.sum(occ_tgt)
        else:
            out_dict['iou' + ext] = 0.
            out_dict['precision' + ext] = float("nan")
            out_dict['recall' + ext] = float("nan")
        return out_dict

    def eval_pointcloud(self, pointcloud, pointcloud_tgt, normals=None, normals_tgt=None, thresholds=DEFAULT_THRESHOLDS):
        if len(pointcloud) == 0:
            return _empty_dict(normals is not None and normals_tgt is not None)
        return self._eval_pointclouds([pointcloud], [pointcloud_tgt], [normals], [normals_tgt], thresholds)[0]

    def _eval_pointclouds(self, clouds, clouds_tgt, normals, normals_tgt, thresholds):
        # completeness: target -> prediction; accuracy: prediction -> target.  Two launches for the whole batch
        comp, ci, co = nn_query_batch(clouds_tgt, clouds)
        acc, ai, ao = nn_query_batch(clouds, clouds_tgt)
        dev = comp.device
        out = []
        for b in range(len(clouds)):
            c, a = comp[co[b]:co[b + 1]], acc[ao[b]:ao[b + 1]]
            if normals[b] is not None and normals_tgt[b] is not None:
                cd = _normal_dots(ci[co[b]:co[b + 1]], normals_tgt[b], normals[b], dev)
                ad = _normal_dots(ai[ao[b]:ao[b + 1]], normals[b], normals_tgt[b], dev)
            else:
                cd = torch.full((len(c),), float("nan"), device=dev)
                ad = torch.full((len(a),), float("nan"), device=dev)
            out.append(_pointcloud_dict(c, cd, a, ad, thresholds))
        return out
