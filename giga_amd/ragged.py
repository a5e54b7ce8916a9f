"""Ragged batches for the library's calls: B meshes or point clouds back to back in one device tensor, with the B + 1 int32 row
offsets on the host (the form `giga_nn_query`, `giga_mesh_sample`, `giga_mesh_contains`, `giga_mesh_collide`, `giga_depth_render`
and `giga_affordance_faces` take).  A mesh is a `giga_amd.mesh.Mesh`, any object with `vertices` and `faces`, or a
`(vertices, faces)` pair of numpy arrays or device tensors."""
import numpy as np
import torch

MAX_ROWS = 2 ** 31 - 1       # the offsets are int32


def mesh_parts(mesh):
    """(vertices, faces) of a mesh in any of its forms"""
    if hasattr(mesh, "vertices") and hasattr(mesh, "faces"):
        return mesh.vertices, mesh.faces
    v, f = mesh
    return v, f


def mesh_arrays(meshes):
    """the vertex and face arrays of a list of meshes, flat: what `_capi.hip_device` looks at"""
    return [x for m in meshes for x in mesh_parts(m)]


def to_device(x, dev, dtype, cols=3):
    """numpy array or device tensor -> contiguous (n, cols) device tensor of `dtype`"""
    if x is None:
        return None
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t = t.detach()
    if cols:
        t = t.reshape(-1, cols)
    return t.to(dtype).contiguous()


def offsets(counts):
    """B counts -> the B + 1 int32 offsets of the batch"""
    o = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=o[1:])
    if o[-1] > MAX_ROWS:
        raise ValueError("a ragged batch holds at most 2^31 - 1 rows")
    return np.ascontiguousarray(o, np.int32)


def pack(items, dev, dtype, cols=3):
    """list of B arrays -> (all rows in one device tensor, offsets)"""
    ts = [to_device(t, dev, dtype, cols) for t in items]
    return (ts[0] if len(ts) == 1 else torch.cat(ts)), offsets([len(t) for t in ts])


def pack_meshes(meshes, dev):
    """list of B meshes -> (vertices float32, vertex offsets, faces int32, face offsets)"""
    parts = [mesh_parts(m) for m in meshes]
    v, vo = pack([p[0] for p in parts], dev, torch.float32)
    f, fo = pack([p[1] for p in parts], dev, torch.int32)
    return v, vo, f, fo
