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
    L = _capi.lib()
    counts_dev = torch.zeros((max(B, 1), 2), dtype=torch.int32, device=dev)
    ws = torch.empty(max(L.giga_mesh_workspace_bytes(B, nx, ny, nz), 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _capi.check(L.giga_mesh_count(_capi.ptr(g), B, nx, ny, nz, float(iso), _capi.ptr(ws), ws.numel(), _capi.ptr(counts_dev),
                                      _capi.stream_ptr(dev)), "giga_mesh_count")
        counts = counts_dev[:B].cpu().to(torch.int64)
        cap_v, cap_t = int(counts[:, 0].sum()), int(counts[:, 1].sum())
        vertices = torch.empty((cap_v, 3), dtype=torch.float32, device=dev)
        triangles = torch.empty((cap_t, 3), dtype=torch.int32, device=dev)
        _capi.check(L.giga_mesh_emit(_capi.ptr(g), B, nx, ny, nz, float(iso), float(box_size), _capi.ptr(ws), ws.numel(),
                                     _capi.ptr(vertices), cap_v, _capi.ptr(triangles), cap_t, None,
                                     _capi.stream_ptr(dev)), "giga_mesh_emit")
    return vertices, triangles, counts
