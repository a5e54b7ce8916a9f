"""Do two triangle meshes intersect?  `mesh_collide` answers it for a list of pairs of bodies in one `giga_mesh_collide` launch
(csrc/giga_collide.hip; the decision is written out in include/giga_hip.h): exact-order double-precision orientation tests of
every edge of one body against every triangle of the other, after bounding-box culling.  Meshes are `(vertices, faces)` pairs of
numpy arrays or device tensors (or objects with these attributes) in world coordinates.  There is no CPU path: CPU tensors raise
`GigaHipError`.

The surface test cannot see a body that lies wholly inside another; `containment=True` adds `giga_mesh_contains` on one vertex of
either body.  Coplanar contact (two faces lying in one plane) is not detected, by definition."""
import numpy as np
import torch

from . import _capi, ragged
from .eval import mesh_contains_batch


def mesh_bounds_batch(meshes):
    """(M, 2, 3) float32 numpy array: the axis-aligned box [min, max] over all vertices of each mesh, taken where the vertices
    live; a mesh without vertices gives (+inf, -inf)."""
    out = np.empty((len(meshes), 2, 3), np.float32)
    out[:, 0], out[:, 1] = np.inf, -np.inf
    for m, mesh in enumerate(meshes):
        v = ragged.mesh_parts(mesh)[0]
        if torch.is_tensor(v):
            v = v.detach().reshape(-1, 3).float()
            if len(v):
                out[m] = torch.stack((v.amin(dim=0), v.amax(dim=0))).cpu().numpy()
        else:
            v = np.asarray(v, np.float32).reshape(-1, 3)
            if len(v):
                out[m, 0], out[m, 1] = v.min(axis=0), v.max(axis=0)
    return out


def _first_vertices(v, vo, f, fo):
    """per body the first vertex its faces use: (points (M, 3) float32 device tensor, usable (M,) bool on the host)"""
    M = len(vo) - 1
    has = fo[1:] > fo[:-1]
    rows = torch.as_tensor(np.where(has, fo[:-1], 0).astype(np.int64), device=v.device)
    first = f[rows, 0].cpu().numpy().astype(np.int64) if len(f) else np.zeros(M, np.int64)
    usable = has & (first >= 0) & (first < vo[1:] - vo[:-1])
    index = torch.as_tensor(np.where(usable, vo[:-1] + first, 0).astype(np.int64), device=v.device)
    points = v[index] if len(v) else torch.zeros((M, 3), dtype=torch.float32, device=v.device)
    return points, usable


def mesh_collide(meshes, pairs, containment=True, device=None):
    """meshes: M bodies; pairs: (P, 2) indices into them, a != b.  Returns a (P,) bool device tensor: do the two surfaces intersect?
    containment=True ORs in two point-in-mesh queries per pair -- the first vertex that body a's faces use against body b, and the
    reverse, all pairs in one `mesh_contains_batch` call (one scene per body that is asked about) -- so that a solid wholly inside
    another solid counts as a collision, while an object standing inside a hollow open mesh does not."""
    dev = _capi.hip_device(*ragged.mesh_arrays(meshes), device=device, what="mesh collision runs on a HIP device")
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    M, P = len(meshes), len(pairs)
    if P and (M == 0 or pairs.min() < 0 or pairs.max() >= M or (pairs[:, 0] == pairs[:, 1]).any()):
        raise ValueError("a pair names two different bodies of the list")
    hit = torch.zeros(P, dtype=torch.uint8, device=dev)
    if P == 0:
        return hit.to(torch.bool)
    v, vo, f, fo = ragged.pack_meshes(meshes, dev)
    ws = _capi.workspace("giga_mesh_collide", dev, M, P)
    _capi.call("giga_mesh_collide", dev, v, vo, f, fo, M, np.ascontiguousarray(pairs, np.int32), P, hit, ws, ws.numel())
    hit = hit.to(torch.bool)
    if not containment:
        return hit
    # query (point of body src) against (mesh of body dst), both directions of every pair, grouped by dst
    points, usable = _first_vertices(v, vo, f, fo)
    src = np.concatenate((pairs[:, 0], pairs[:, 1]))
    dst = np.concatenate((pairs[:, 1], pairs[:, 0]))
    row = np.concatenate((np.arange(P), np.arange(P)))
    ask = usable[src] & (fo[1:] > fo[:-1])[dst]
    src, dst, row = src[ask], dst[ask], row[ask]
    if not len(src):
        return hit
    order = np.argsort(dst, kind="stable")
    src, dst, row = src[order], dst[order], row[order]
    bodies, counts = np.unique(dst, return_counts=True)
    queries = points[torch.as_tensor(src, device=dev)]
    inside, _ = mesh_contains_batch([(v[vo[b]:vo[b + 1]], f[fo[b]:fo[b + 1]]) for b in bodies],
                                    list(torch.split(queries, counts.tolist())))
    return _or_rows(hit, row, inside)


def _or_rows(hit, row, inside):
    """hit[row[k]] |= inside[k] (a row may appear twice)"""
    extra = torch.zeros(len(hit), dtype=torch.int32, device=hit.device)
    extra.index_add_(0, torch.as_tensor(row, device=hit.device), inside.to(torch.int32))
    return hit | (extra > 0)
