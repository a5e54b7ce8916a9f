"""Marching cubes on device-resident value grids (csrc/giga_mesh.hip through giga_mesh_count / giga_mesh_emit) and the
`Mesh` record that `Generator3D` returns in place of `trimesh.Trimesh` (trimesh is an optional dependency)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import _capi


@dataclass
class Mesh:
    """vertices (V,3) float32, faces (F,3) int64, vertex_normals (V,3) float32 or None: numpy arrays like the ones the
    reference hands to `trimesh.Trimesh(vertices, triangles, vertex_normals=normals, process=False)`."""
    vertices: np.ndarray
    faces: np.ndarray
    vertex_normals: Optional[np.ndarray] = None

    @classmethod
    def empty(cls):
        return cls(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64), None)

    def to_trimesh(self):
        import trimesh                       # optional: raises ImportError where it is not installed
        return trimesh.Trimesh(self.vertices, self.faces, vertex_normals=self.vertex_normals, process=False)


def marching_cubes(grids, iso, box_size=1.0):
    """grids (B,nx,ny,nz) fp32 on the device -> (vertices (V,3) fp32, triangles (F,3) int32, counts (B,2) int64 on the host).
    Scenes are packed back to back in scene order; a scene's triangles index from its own first vertex.  The ONLY
    device-to-host traffic is `counts` (one copy of B x 2 int32, which is also the only synchronisation)."""
    if grids.dim() != 4:
        raise ValueError(f"expected (B,nx,ny,nz) grids, got {tuple(grids.shape)}")
    dev = _capi.device_of(grids)
    g = grids.detach().contiguous().float()
    B, nx, ny, nz = g.shape
    counts_dev = torch.zeros((max(B, 1), 2), dtype=torch.int32, device=dev)
    ws = _capi.workspace("giga_mesh", dev, B, nx, ny, nz)
    _capi.call("giga_mesh_count", dev, g, B, nx, ny, nz, float(iso), ws, ws.numel(), counts_dev)
    counts = counts_dev[:B].cpu().to(torch.int64)
    cap_v, cap_t = int(counts[:, 0].sum()), int(counts[:, 1].sum())
    vertices = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((cap_t, 3), dtype=torch.int32, device=dev)
    _capi.call("giga_mesh_emit", dev, g, B, nx, ny, nz, float(iso), float(box_size), ws, ws.numel(), vertices, cap_v, triangles, cap_t,
               None)
    return vertices, triangles, counts


def simplify_mesh(vertices, faces, f_target, agressiveness=7., counts=None, stats=None, ref_extra=None):
    """The reference's `simplify_mesh(mesh, f_target, agressiveness)` (utils/libsimplify: the greedy quadric edge collapse of
    Simplify.h) on device-resident meshes, face for face and vertex for vertex in float64 (csrc/giga_simplify.hip through
    giga_mesh_simplify).  vertices (V,3) float32 or float64 and faces (F,3) integer tensors on the device; one mesh, or with
    `counts` (B,2) = {#vertices, #faces} per mesh, B meshes back to back as `marching_cubes` returns them (a mesh's faces count
    from its own first vertex).  f_target: an int, or one int per mesh.  Returns device tensors (vertices (V',3) float64, faces
    (F',3) of the dtype given, counts (B,2) int64) in the same layout.  A mesh with no more than f_target faces comes back with
    its unreferenced vertices dropped, an empty mesh comes back empty.  `stats` (a dict) receives "iterations", "rounds",
    "repeated passes" and "list rebuilds", one int per mesh.  `ref_extra`: room of the per-vertex reference lists beyond 3 F
    entries per mesh (default 3 F + 64; not below `_capi.SIMPLIFY_MIN_REF_EXTRA`), which changes how often the lists are rebuilt
    and nothing else.  There is no CPU path: a host tensor raises GigaHipError.  The call reads the pending counts back between
    rounds, so it returns with the result computed."""
    if vertices.dim() != 2 or vertices.shape[-1] != 3 or faces.dim() != 2 or faces.shape[-1] != 3:
        raise ValueError(f"expected (V,3) vertices and (F,3) faces, got {tuple(vertices.shape)} and {tuple(faces.shape)}")
    dev = _capi.device_of(vertices, faces)
    if counts is None:
        counts_h = torch.tensor([[vertices.shape[0], faces.shape[0]]], dtype=torch.int64)
    else:
        counts_h = torch.as_tensor(counts).detach().cpu().to(torch.int64).reshape(-1, 2)
    B = counts_h.shape[0]
    if int(counts_h[:, 0].sum()) != vertices.shape[0] or int(counts_h[:, 1].sum()) != faces.shape[0] or bool((counts_h < 0).any()):
        raise ValueError("counts do not add up to the vertices and faces given")
    targets = torch.as_tensor(f_target, dtype=torch.int64).reshape(-1).cpu()
    targets = targets.expand(B) if targets.numel() == 1 else targets
    if targets.numel() != B:
        raise ValueError(f"expected one f_target or one per mesh ({B}), got {targets.numel()}")
    targets = targets.clamp(max=2 ** 31 - 1).to(torch.int32).contiguous()
    v = vertices.detach().contiguous()
    if v.dtype != torch.float64:
        v = v.float()
    f = faces.detach().to(torch.int32).contiguous()
    zero = torch.zeros((1, 1), dtype=torch.int64)
    voff = torch.cat((zero, counts_h[:, :1].cumsum(0))).to(torch.int32).reshape(-1).contiguous()
    foff = torch.cat((zero, counts_h[:, 1:].cumsum(0))).to(torch.int32).reshape(-1).contiguous()
    extra = -1 if ref_extra is None else int(ref_extra)
    out_v = torch.empty((v.shape[0], 3), dtype=torch.float64, device=dev)
    out_f = torch.empty((f.shape[0], 3), dtype=torch.int32, device=dev)
    out_c = torch.zeros((max(B, 1), 2), dtype=torch.int32, device=dev)
    st = torch.zeros((max(B, 1), 4), dtype=torch.int32)
    ws = _capi.workspace("giga_simplify", dev, B, v.shape[0], f.shape[0], extra)       # (0 bytes for a shape the call rejects)
    _capi.call("giga_mesh_simplify", dev, v, int(v.dtype == torch.float64), voff, f, foff, targets, B, float(agressiveness), extra,
               out_v, out_f, out_c, st, ws, ws.numel())
    out_counts = out_c[:B].to(torch.int64)
    totals = out_counts.sum(0).tolist() if B else [0, 0]
    if stats is not None:
        for k, name in enumerate(("iterations", "rounds", "repeated passes", "list rebuilds")):
            stats[name] = st[:B, k].tolist()
    return out_v[:totals[0]], out_f[:totals[1]].to(faces.dtype), out_counts
