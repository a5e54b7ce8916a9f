"""Mesh refinement on the device: the reference's `Generator3D.refine_mesh` (conv_onet/generation.py:457-519).

The reference draws one point per face (Dirichlet(1/2,1/2,1/2) barycentric weights), pulls it onto the network's iso-surface
(`(sigmoid(f) - threshold)^2`) and aligns the face normal with `-grad sigmoid(f)` (`0.01 |n - t|^2`), by RMSprop(lr=1e-4) on the
vertices.  Its gradient needs the second derivative of the occupancy logit w.r.t. the query point, which it asks of autograd
through `F.grid_sample` (`create_graph=True`).  Here the Hessian comes out of the point-gradient kernel (three numbers per point:
the heads are piecewise linear and the sample bilinear, `convonet.decoder_point_hess`), and the gradient of the loss is closed-form
per-face arithmetic (csrc/giga_refine.hip).  A step is four launches and nothing leaves the device."""
import torch

from . import _capi
from .convonet import _planes_to_nhwc, decoder_point_hess


class MeshRefiner:
    """Refinement state of ONE mesh on the planes `c` of ONE scene.  vertices (V,3) float, faces (F,3) integer, tensors on the
    device or arrays.  `step(eps=None)` runs one optimiser step -- face points (weights `eps` (F,3) if given, else drawn from
    `(seed, step index, face)`), logit / gradient / Hessian at them, face gradients, vertex step -- and leaves on the device:
    `vertices` (V,3), `grad` (V,3), `square_avg` (V,3), `eps` (F,3), `face_points` (F,3), `face_grad` (F,3,3) and `loss` (2,) =
    (loss_target, loss_normal) of the step's start.  The same `(seed, vertices, faces, planes)` give the same bits on every run."""

    def __init__(self, model, c, vertices, faces, threshold=0.5, seed=0):
        nhwc = c if torch.is_tensor(c) else _planes_to_nhwc(c, "fp32")         # (a tensor: fp32 NHWC planes [3,1,40,40,32])
        dev = _capi.device_of(nhwc)
        if nhwc.dtype != torch.float32 or nhwc.dim() != 5:
            raise ValueError("MeshRefiner reads fp32 NHWC planes [3,1,40,40,32]")
        if nhwc.shape[1] != 1:
            raise ValueError(f"MeshRefiner takes the planes of one scene, got {nhwc.shape[1]}")
        if not 0.0 < float(threshold) < 1.0:
            raise ValueError(f"threshold must lie inside (0, 1), got {threshold}")
        self.nhwc = nhwc.contiguous()
        self.blob, self.bwd_blob = model.packed_blob(dev), model.packed_bwd_blob(dev)
        self.threshold, self.seed, self.steps = float(threshold), int(seed), 0
        v = torch.as_tensor(vertices).to(dev, torch.float32)
        f = torch.as_tensor(faces).to(dev)
        if v.dim() != 2 or v.shape[-1] != 3 or f.dim() != 2 or f.shape[-1] != 3:
            raise ValueError(f"expected (V,3) vertices and (F,3) faces, got {tuple(v.shape)} and {tuple(f.shape)}")
        V, F = v.shape[0], f.shape[0]
        if max(V, F) > _capi.REFINE_MAX_FACES:
            raise ValueError("mesh too large for one refinement call")
        if F and (int(f.min()) < 0 or int(f.max()) >= V):          # (the one synchronisation: the kernels trust no index either)
            raise ValueError("face index outside the vertex array")
        self.vertices = v.clone().contiguous()
        self.faces = f.to(torch.int32).contiguous()
        # corners (3 face + i) sorted by vertex, CSR: the topology is fixed, the summation order with it
        flat = self.faces.reshape(-1).long()
        self.corner_order = torch.sort(flat, stable=True)[1].to(torch.int32).contiguous()
        self.vertex_offsets = torch.zeros(V + 1, dtype=torch.int32, device=dev)
        if F:
            self.vertex_offsets[1:] = torch.bincount(flat, minlength=V).cumsum(0).to(torch.int32)
        self.grad = torch.zeros((V, 3), device=dev)
        self.square_avg = torch.zeros((V, 3), device=dev)
        self.eps = torch.empty((F, 3), device=dev)
        self.face_points = torch.empty((F, 3), device=dev)
        self.face_loss = torch.zeros((F, 2), device=dev)
        self.face_grad = torch.zeros((F, 3, 3), device=dev)
        self.logit = self.dp = self.hess = None

    @property
    def loss(self):
        """(loss_target, loss_normal) of the last step: the means over the faces, fixed summation order."""
        if self.face_loss.shape[0] == 0:
            return torch.zeros(2, device=self.face_loss.device)
        return self.face_loss.double().mean(0).float()

    def step(self, eps=None):
        V, F = self.vertices.shape[0], self.faces.shape[0]
        dev = self.vertices.device
        eps_in = None
        if eps is not None:
            eps_in = torch.as_tensor(eps).to(dev, torch.float32).contiguous()
            if tuple(eps_in.shape) != (F, 3):
                raise ValueError(f"expected ({F},3) barycentric weights, got {tuple(eps_in.shape)}")
        with torch.no_grad(), torch.cuda.device(dev):
            _capi.call("giga_refine_face_points", dev, self.vertices, self.faces, eps_in, self.eps, self.face_points, V, F, self.seed,
                       self.steps)
            self.logit, self.dp, self.hess = (t[0] for t in decoder_point_hess(self.nhwc, self.face_points[None], self.blob,
                                                                              self.bwd_blob))
            _capi.call("giga_refine_face_grad", dev, self.vertices, self.faces, self.eps, self.logit, self.dp, self.hess,
                       self.threshold, self.face_loss, self.face_grad, V, F)
            _capi.call("giga_refine_vertex_step", dev, self.face_grad, self.corner_order, self.vertex_offsets, self.vertices,
                       self.square_avg, self.grad, V, F)
        self.steps += 1
        return self

    def run(self, n):
        for _ in range(int(n)):
            self.step()
        return self.vertices
