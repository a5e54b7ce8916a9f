"""Occupancy / geometry query path: counterpart of `Generator3D.eval_points` and the dense-grid part of
`generate_from_latent` (/root/reference/src/vgn/ConvONets/conv_onet/generation.py:326-358, 144-190), SURVEY.md
section 8f-2.

The reference splits the query set into `points_batch_size` chunks, moves each chunk to the device, calls
`model.decode_occ(pi, c).logits` and copies every chunk back.  Here the planes stay cached on the device in the
layout the decoder reads (`PlaneDict.nhwc`, produced once by `encode_inputs`), the fused decoder takes a whole
chunk in ONE launch (there is no activation tensor whose size would call for chunking: `points_batch_size` only bounds
the device copy of a HOST-resident query set, one chunk in flight at a time), and a regular grid of
queries takes the lattice path (each plane sampled once per lattice coordinate pair).

Mesh extraction (`generate_mesh`, `generate_from_latent`, `extract_mesh`, generation.py:68-148, 360-428) runs on the device
too: marching cubes is csrc/giga_mesh.hip (the reference pads the grid on the host and calls libmcubes), the vertices stay
on the device for `estimate_normals`, and the only device-to-host traffic before the final copy of the mesh is the B x 2
vertex / triangle counts.  The value grid has the shape of MISE's `to_dense()` -- resolution0 * 2**upsampling_steps + 1 samples
per axis, 129^3 by default -- and is filled in one of two ways.  By default (`mise=False`) every sample is decoded, in one launch;
the mesh then equals the reference's wherever MISE evaluated every sample next to the surface, and it can contain components
smaller than a coarse cell, which MISE skips.  With `mise=True` (and upsampling_steps > 0) the grid is the reference's: MISE
(utils/libmise/mise.pyx) runs on the device (`giga_amd.mise`, csrc/giga_mise.hip), bit for bit libmise's bookkeeping -- decode the
coarse lattice, subdivide only voxels that see both sides of the threshold, repeat, `to_dense()` -- with one decoder launch per
round over all scenes and the B list lengths as the only device-to-host traffic of a round; it is also the route to the grids the
dense one cannot afford (257^3, 513^3).

Mesh refinement (`refinement_step`, generation.py:457-519) runs on the device as well (`giga_amd.refine`, csrc/giga_refine.hip):
per scene, `refinement_step` RMSprop steps of four launches each on the vertices marching cubes left on the device, before the
final copy.  The second derivative of the occupancy logit that the reference asks of autograd through `F.grid_sample` (a double
backward current torch builds do not implement) is three numbers per face point from the point-gradient kernel.

Mesh simplification (`simplify_nfaces`, generation.py:417-420: `simplify_mesh(mesh, simplify_nfaces, 5.)`, the quadric edge collapse
of utils/libsimplify/Simplify.h) runs on the device too (`giga_amd.mesh.simplify_mesh`, csrc/giga_simplify.hip): after the normals,
all scenes in one call, the reference's mesh face for face and vertex for vertex in float64 (cast to float32 where the `Mesh` leaves
the device).  A simplified mesh carries no vertex normals ("normals are lost here", generation.py:419).  `simplify_nfaces` together
with `refinement_step > 0` in ONE generator is not built; the two-call route works: simplify with one generator, then
`Generator3D(net, refinement_step=k).refine_mesh(mesh, c=c)`.  The crop mode (`vol_bound`) is not built."""
import time

import numpy as np
import torch

from . import _capi
from .convonet import _planes_to_nhwc, decoder_point_grad, register_lattice
from .mesh import Mesh, marching_cubes, simplify_mesh
from .mise import lin_table, mise_grid
from .refine import MeshRefiner


class Generator3D:
    """generation.py:22-75 (the arguments that matter for the voxel-input GIGA models)."""

    def __init__(self, model, points_batch_size=100000, threshold=0.5, device=None, resolution0=16, upsampling_steps=3,
                 with_normals=False, padding=0.1, refinement_step=0, simplify_nfaces=None, sample=False, input_type=None,
                 vol_info=None, vol_bound=None, mise=False, refine_seed=0):
        """The reference's arguments by name (generation.py:42-49).  `refinement_step > 0` runs that many refinement steps on
        every extracted mesh (`refine_mesh`); it has no CPU path and raises here for a device that is not a HIP device.
        `refine_seed` keys the barycentric draws (the reference uses numpy's global generator).  `simplify_nfaces=N` simplifies
        every extracted mesh to at most N faces (quadric edge collapse, agressiveness 5, module docstring); it has no CPU path
        either and raises here for a device that is not a HIP device, and so does its combination with `refinement_step > 0`,
        which is not built (simplify with one generator, then `Generator3D(net, refinement_step=k).refine_mesh(mesh, c=c)`).
        `vol_bound` (crop mode) raises when a mesh is asked for.  `mesh_options`
        records the mesh arguments as a dict.  `mise=True` fills the value grid by MISE as the reference does (module
        docstring); the default decodes every sample."""
        device = device if device is not None else torch.device("cuda")
        if refinement_step > 0 and torch.device(device).type != "cuda":
            raise NotImplementedError("mesh refinement runs only on a HIP device")
        if refinement_step < 0:                                # (as before: every non-zero value that is not served raises)
            raise NotImplementedError("a negative refinement_step is not built")
        if simplify_nfaces is not None:
            if torch.device(device).type != "cuda":
                raise NotImplementedError("mesh simplification runs only on a HIP device")
            if refinement_step > 0:
                raise NotImplementedError("simplify_nfaces together with refinement_step > 0 is not built: simplify with one "
                                          "generator, then Generator3D(net, refinement_step=k).refine_mesh(mesh, c=c)")
            if int(simplify_nfaces) < 0:
                raise ValueError("simplify_nfaces must not be negative")
        mesh_options = dict(upsampling_steps=upsampling_steps, with_normals=with_normals, padding=padding,
                            refinement_step=refinement_step, simplify_nfaces=simplify_nfaces, sample=sample,
                            input_type=input_type, vol_info=vol_info, vol_bound=vol_bound)
        self.model = model
        self.points_batch_size = int(points_batch_size)
        self.threshold = threshold
        self.refinement_step = int(refinement_step)
        self.refine_seed = int(refine_seed)
        self.device = device
        self.resolution0 = resolution0
        self.upsampling_steps = int(upsampling_steps)
        self.with_normals = bool(with_normals)
        self.padding = padding
        self.simplify_nfaces = int(simplify_nfaces) if simplify_nfaces is not None else None
        self.mesh_options = dict(mesh_options)
        self.mise = bool(mise)
        self._grids = {}

    def encode(self, inputs):
        """generation.py:99-101: c = model.encode_inputs(inputs), kept on the device for every later query."""
        with torch.no_grad():
            return self.model.encode_inputs(inputs.to(self.device))

    def eval_points(self, p, c=None, **kwargs):
        """generation.py:326-358 (`else` branch: voxel / point-cloud inputs).  p: (N,3) or (B,N,3) points in the
        unit cube, on any device; returns the occupancy logits on the device, (N,) or (B,N).  One launch; the
        reference's chunk loop and per-chunk D->H copy disappear (use `.cpu()` for its return type)."""
        squeeze = p.dim() == 2
        pts = p.unsqueeze(0) if squeeze else p
        with torch.no_grad():
            if pts.is_cuda or pts.shape[1] <= self.points_batch_size:
                logits = self.model.decode_occ(pts.to(self.device, torch.float32), c, **kwargs).logits
            else:                                             # host-resident queries: bounded device footprint (generation.py:337)
                parts = [self.model.decode_occ(ch.to(self.device, torch.float32), c, **kwargs).logits
                         for ch in torch.split(pts, self.points_batch_size, dim=1)]
                logits = torch.cat(parts, dim=1)
        return logits.squeeze(0) if squeeze else logits

    def estimate_normals(self, vertices, c=None):
        """generation.py:430-455: normals = -grad_p(occupancy logit) / |.| at the mesh vertices.  vertices: (N,3) numpy array
        or tensor; c: the planes of ONE scene (`encode`).  Returns a numpy (N,3) float32 array, as the reference does.  The
        gradient is one giga_decoder_point_grad launch (occupancy head, fp32) per chunk; like `eval_points`, only a
        host-resident vertex set is split into `points_batch_size` chunks.  Unlike the reference's `backward()`, nothing
        is accumulated into the parameters' `.grad`."""
        v = torch.from_numpy(np.asarray(vertices, dtype=np.float32)) if not torch.is_tensor(vertices) else vertices
        if v.dim() != 2 or v.shape[-1] != 3:
            raise ValueError(f"expected (N,3) vertices, got {tuple(v.shape)}")
        with torch.no_grad():
            nhwc = _planes_to_nhwc(c, "fp32")
            chunks = [v] if v.is_cuda or v.shape[0] <= self.points_batch_size else torch.split(v, self.points_batch_size)
            normals = [self._normals_on_device(vi.to(self.device, torch.float32), nhwc).cpu().numpy() for vi in chunks]
        return np.concatenate(normals, axis=0) if normals else np.zeros((0, 3), np.float32)

    def _normals_on_device(self, v, nhwc):
        """`estimate_normals` for device-resident vertices (N,3) and the fp32 NHWC planes of one scene; the result stays on
        the device (the mesh path copies vertices and normals to the host together, once)."""
        blob, bwd_blob = self.model.packed_blob(nhwc.device), self.model.packed_bwd_blob(nhwc.device)
        vi = v.unsqueeze(0)
        ones = torch.ones(vi.shape[:-1], device=vi.device)
        ni = -decoder_point_grad(nhwc, vi, blob, bwd_blob, 8, {"decoder_tsdf": ones})
        return (ni / torch.norm(ni, dim=-1, keepdim=True)).squeeze(0)

    def grid_points(self, resolution, lo=-0.5, hi=0.5):
        """The (1, R^3, 3) regular grid `box_size * make_3d_grid((-0.5,)*3, (0.5,)*3, (R,)*3)` of generation.py:160-165
        (box_size folded into lo/hi), registered as a lattice so that decoding it takes the lattice path."""
        key = (int(resolution), float(lo), float(hi))
        g = self._grids.get(key)
        if g is None:
            lin = torch.linspace(lo, hi, resolution)
            x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
            pts = torch.stack((x, y, z), dim=-1).float().reshape(1, resolution ** 3, 3).to(self.device)
            g = self._grids[key] = register_lattice(pts, lin)
        return g

    def occupancy_grid(self, c, resolution=None, lo=-0.5, hi=0.5):
        """generation.py:157-166 (upsampling_steps == 0): logits on the dense R^3 grid -> (B,R,R,R) device tensor."""
        if resolution is None:
            resolution = self.resolution0
        if resolution > 64:
            raise _capi.GigaHipError("the lattice decoder supports up to 64 points per axis; use eval_points")
        with torch.no_grad():
            logits = self.model.decode_occ(self.grid_points(resolution, lo, hi), c).logits
        return logits.view(-1, resolution, resolution, resolution)

    # ---- mesh extraction (generation.py:68-148, 360-428) ---------------------------------------------------------------
    def grid_resolution(self):
        """Samples per axis of the value grid: resolution0 for upsampling_steps == 0 (generation.py:117-124), else the
        shape of MISE.to_dense(), resolution0 * 2**upsampling_steps + 1."""
        return self.resolution0 if self.upsampling_steps == 0 else self.resolution0 * 2 ** self.upsampling_steps + 1

    def _mesh_points(self, n, box_size):
        """(1, n^3, 3): `box_size * make_3d_grid((-0.5,)*3, (0.5,)*3, (n,)*3)` with the reference's fp32 arithmetic (the
        product is rounded after linspace, generation.py:119-121); registered as a lattice where the lattice decoder applies."""
        key = ("mesh", int(n), float(box_size))
        g = self._grids.get(key)
        if g is None:
            lin = box_size * torch.linspace(-0.5, 0.5, n)
            x, y, z = torch.meshgrid(lin, lin, lin, indexing="ij")
            g = torch.stack((x, y, z), dim=-1).float().reshape(1, n ** 3, 3).to(self.device)
            self._grids[key] = register_lattice(g, lin) if n <= 64 else g
        return g

    def mise_lin(self):
        """The per-axis coordinate table of the MISE lattice (generation.py:132-135), float32 [grid_resolution()] on the host."""
        return lin_table(self.resolution0 << self.upsampling_steps, 1 + self.padding)

    def value_grid(self, c, stats_dict=None):
        """Occupancy logits of every scene of `c`, (B,n,n,n) on the device, n = `grid_resolution()`.  Default: every sample of the
        grid of `_mesh_points(n, 1 + padding)`; up to 64 samples per axis take the lattice decoder, larger grids the generic
        decoder in one launch over all scenes.  `mise=True` with upsampling_steps > 0: MISE's `to_dense()` grid, one generic-decoder
        launch per round over the ragged query lists of all scenes (padded to the longest); `stats_dict` receives "mise rounds"
        and "mise points"."""
        if self.mise and self.upsampling_steps > 0:
            key = ("mise", self.resolution0, self.upsampling_steps, float(self.padding))
            lin = self._grids.get(key)
            if lin is None:
                lin = self._grids[key] = torch.from_numpy(self.mise_lin()).to(self.device)
            return mise_grid(lambda q, pts: self.eval_points(pts, c), self.resolution0, self.upsampling_steps, self._iso(),
                             batch=self._scenes(c), device=lin.device, lin=lin, stats=stats_dict)
        n = self.grid_resolution()
        p = self._mesh_points(n, 1 + self.padding)
        B = self._scenes(c)
        if n > 64:
            p = p.expand(B, -1, -1)
        return self.eval_points(p, c).view(B, n, n, n)

    @staticmethod
    def _scenes(c):
        """Number of scenes of the planes `c` (a PlaneDict of `encode`, or a reference-style dict of (B,32,40,40) tensors)."""
        nhwc = getattr(c, "nhwc", None)
        return int(nhwc.shape[1]) if nhwc is not None else int(next(iter(c.values())).shape[0])

    def _iso(self):
        return float(np.log(self.threshold) - np.log(1. - self.threshold))

    def _meshes(self, grids, c, stats_dict):
        """Marching cubes over (B,n,n,n) device grids (+ normals): one set of launches, then one copy per array and scene."""
        if not torch.is_tensor(grids) or not grids.is_cuda:
            raise _capi.GigaHipError("mesh extraction runs only on a HIP device (the value grid must be a device tensor); "
                                     "there is no CPU fallback")
        if self.mesh_options.get("vol_bound") is not None:
            raise NotImplementedError("the crop mode (vol_bound) is not built")
        if grids.shape[0] == 0:
            return []
        t0 = time.time()
        vertices, triangles, counts = marching_cubes(grids, self._iso(), 1 + self.padding)
        stats_dict["time (marching cubes)"] = time.time() - t0
        v_end, t_end = counts[:, 0].cumsum(0).tolist(), counts[:, 1].cumsum(0).tolist()
        normals = None
        if self.with_normals and v_end[-1] > 0:
            t0 = time.time()
            with torch.no_grad():
                nhwc = _planes_to_nhwc(c, "fp32")
                normals = torch.empty_like(vertices)
                for b, (v1, nv) in enumerate(zip(v_end, counts[:, 0].tolist())):
                    if nv:
                        normals[v1 - nv:v1] = self._normals_on_device(vertices[v1 - nv:v1], nhwc[:, b:b + 1].contiguous())
            stats_dict["time (normals)"] = time.time() - t0
        if self.simplify_nfaces is not None and t_end[-1] > 0:
            # generation.py:417-420: after the normals, which belong to the vertices of the full mesh ("normals are lost here").
            # All scenes in one call (they share their rounds); an empty mesh passes through as it is.
            t0 = time.time()
            vertices, triangles, counts = simplify_mesh(vertices, triangles, self.simplify_nfaces, 5., counts=counts)
            counts = counts.cpu()
            v_end, t_end = counts[:, 0].cumsum(0).tolist(), counts[:, 1].cumsum(0).tolist()
            vertices, normals = vertices.float(), None
            stats_dict["time (simplify)"] = time.time() - t0
        if self.refinement_step > 0 and v_end[-1] > 0:
            # generation.py:423-426: after the normals, which belong to the unrefined vertices and are lost with them (trimesh
            # drops its cached vertex normals when `mesh.vertices` is assigned): a refined mesh carries none
            t0 = time.time()
            nhwc = _planes_to_nhwc(c, "fp32")
            for b, (v1, nv) in enumerate(zip(v_end, counts[:, 0].tolist())):
                nt = int(counts[b, 1])
                if nv and nt:
                    vertices[v1 - nv:v1] = self._refine_on_device(vertices[v1 - nv:v1], triangles[t_end[b] - nt:t_end[b]],
                                                                  nhwc[:, b:b + 1])
            normals = None
            stats_dict["time (refine)"] = time.time() - t0
        vertices, faces = vertices.cpu().numpy(), triangles.cpu().numpy().astype(np.int64)
        normals = normals.cpu().numpy() if normals is not None else None
        out = []
        for b in range(grids.shape[0]):
            v0, f0 = v_end[b] - int(counts[b, 0]), t_end[b] - int(counts[b, 1])
            if v_end[b] == v0:
                out.append(Mesh.empty())                       # generation.py:412-414: an empty mesh is returned as it is
                continue
            out.append(Mesh(vertices[v0:v_end[b]], faces[f0:t_end[b]], normals[v0:v_end[b]] if normals is not None else None))
        return out

    def extract_mesh(self, occ_hat, c=None, stats_dict=None):
        """generation.py:360-428: occ_hat (nx,ny,nz) logits ON THE DEVICE -> Mesh in the model's coordinates,
        `box_size * (index / (n - 1) - 0.5)`; vertex normals when `with_normals` (c: the planes of this scene)."""
        if torch.is_tensor(occ_hat) and occ_hat.dim() != 3:
            raise ValueError(f"expected an (nx,ny,nz) grid, got {tuple(occ_hat.shape)}")
        return self._meshes(occ_hat.unsqueeze(0) if torch.is_tensor(occ_hat) else occ_hat, c,
                            stats_dict if stats_dict is not None else {})[0]

    def _refine_on_device(self, vertices, faces, nhwc):
        """`refinement_step` steps on device-resident (V,3) vertices / (F,3) faces of one scene (fp32 NHWC planes); returns the
        refined vertices, on the device."""
        return MeshRefiner(self.model, nhwc, vertices, faces, threshold=self.threshold, seed=self.refine_seed) \
            .run(self.refinement_step)

    def refine_mesh(self, mesh, occ_hat=None, c=None):
        """generation.py:457-519: `refinement_step` RMSprop steps on the vertices of `mesh` (a `Mesh`; c: the planes of its
        scene), which is changed in place and returned; its vertex normals, which belonged to the old vertices, are dropped.
        `occ_hat` is accepted for the reference's signature (it only asserts a cubic grid there).  The mesh path of
        `extract_mesh` does not come through here: it refines before the mesh leaves the device."""
        if self.refinement_step <= 0 or len(mesh.vertices) == 0 or len(mesh.faces) == 0:
            return mesh
        nhwc = _planes_to_nhwc(c, "fp32")
        v = self._refine_on_device(torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float32)).to(nhwc.device),
                                   torch.from_numpy(np.ascontiguousarray(mesh.faces)).to(nhwc.device), nhwc)
        mesh.vertices = v.cpu().numpy()
        mesh.vertex_normals = None
        return mesh

    def generate_from_latent(self, c=None, stats_dict=None, **kwargs):
        """generation.py:102-148; the value grid is dense by default and MISE's with `mise=True` (module docstring)."""
        if self._scenes(c) != 1:
            raise ValueError("generate_from_latent takes the planes of one scene; use generate_meshes for a batch")
        stats_dict = stats_dict if stats_dict is not None else {}
        t0 = time.time()
        grid = self.value_grid(c, stats_dict)
        stats_dict["time (eval points)"] = time.time() - t0
        return self.extract_mesh(grid[0], c, stats_dict=stats_dict)

    def generate_mesh(self, data, return_stats=True):
        """generation.py:68-100: data["inputs"] (1,40,40,40) TSDF -> Mesh (and the stats dict).  The times are host times of
        asynchronous launches; the count readback inside marching cubes is the first point that waits for the device."""
        self.model.eval()
        stats_dict = {}
        t0 = time.time()
        c = self.encode(data["inputs"])
        stats_dict["time (encode inputs)"] = time.time() - t0
        mesh = self.generate_from_latent(c, stats_dict=stats_dict)
        return (mesh, stats_dict) if return_stats else mesh

    def generate_meshes(self, tsdf_batch):
        """B scenes (B,40,40,40) -> list of B meshes: one encoder call, one value-grid launch, one set of marching-cubes
        launches.  Marching cubes and the normals are independent of the batch, so mesh b differs from `generate_mesh` on
        scene b alone only as far as the planes do: byte for byte equal in the precisions whose encoder is independent of the
        batch size (fp16x3, fp16); in fp32, whose encoder's summation order follows the batch, the
        value grids agree at rounding level (well inside the 1e-4 fp32 tolerance), so the vertices move by that much and
        an edge whose end lies that close to the threshold may be crossed in one mesh and not in the other."""
        self.model.eval()
        c = self.encode(tsdf_batch)
        return self._meshes(self.value_grid(c), c, {})
