"""Test-side float64 restatement of the mesh refinement loss (the formulas of include/giga_hip.h; the reference forms the loss at
conv_onet/generation.py:488-511) over pgrad_ref.mlp64.  The reference differentiates `F.grid_sample` twice, which current torch builds do not implement
(`grid_sampler_2d_backward` has no derivative); the bilinear sampler is therefore written here in plain torch ops -- floor, gather,
lerp and the clamp of `normalize_coordinate` -- so that autograd goes through it twice.  Test infrastructure only."""
import torch

import pgrad_ref
from oracle import giga_oracle as O

_AXES = {"xz": (0, 2), "xy": (0, 1), "yz": (1, 2)}          # (grid x, grid y) of common.py:238-261
HEAD = "decoder_tsdf"


def sample_plane(p, c, plane):
    """oracle.sample_plane_feature (grid_sample: bilinear, border, align_corners=True) in plain ops.  p (B,N,3), c (B,C,R,R)
    in the dtype of p -> (B,C,N)."""
    B, C, R, _ = c.shape
    a0, a1 = _AXES[plane]
    xy = torch.stack((p[..., a0], p[..., a1]), dim=-1)
    xy = xy / (1 + 10e-6) + 0.5
    xy = torch.where(xy >= 1, torch.full_like(xy, 1 - 10e-6), xy)
    xy = torch.where(xy < 0, torch.zeros_like(xy), xy)
    f = xy * (R - 1)
    i0 = f.detach().floor().clamp(0, R - 2)
    w = f - i0
    x0, y0 = i0[..., 0].long(), i0[..., 1].long()
    flat = c.reshape(B, C, R * R)

    def tap(iy, ix):
        return flat.gather(2, (iy * R + ix)[:, None, :].expand(B, C, -1))

    wx, wy = w[..., 0][:, None, :], w[..., 1][:, None, :]
    f00, f01, f10, f11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = f00 + wx * (f01 - f00)
    bot = f10 + wx * (f11 - f10)
    return top + wy * (bot - top)


def sample_features(p, planes):
    """oracle.sample_features: (B,N,96) in the order xz, xy, yz."""
    return torch.cat([sample_plane(p, planes[k], k) for k in O.PLANES], dim=1).transpose(1, 2)


def logits(sd, planes, p, pre=None):
    """Occupancy logits (B,N) at p (B,N,3), in the dtype of p; `pre` collects every ReLU input."""
    return pgrad_ref.mlp64(sd, HEAD, p, sample_features(p, planes), pre)


def cast_planes(planes, dtype=torch.float64):
    return {k: v.detach().to(dtype) for k, v in planes.items()}


def point_hess(sd, planes, p, pre=None, dtype=torch.float64):
    """(logit (B,N), grad (B,N,3), hessian (B,N,3,3)) of the occupancy logit w.r.t. p by double autograd."""
    pl = cast_planes(planes, dtype)
    q = p.detach().to(dtype).clone().requires_grad_(True)
    f = logits(sd, pl, q, pre)
    (g,) = torch.autograd.grad(f.sum(), q, create_graph=True)
    rows = []
    for i in range(3):
        if g.requires_grad and g.grad_fn is not None:
            (r,) = torch.autograd.grad(g[..., i].sum(), q, retain_graph=True, allow_unused=True)
            rows.append(r if r is not None else torch.zeros_like(q))
        else:
            rows.append(torch.zeros_like(q))
    return f.detach(), g.detach(), torch.stack(rows, dim=-2)


def _unit(a):
    """a / (|a| + 1e-10) row by row: the guarded normalisation of both normals."""
    return a / (a.norm(dim=1, keepdim=True) + 1e-10)


def corner_loss(sd, planes, corners, eps, threshold=0.5, pre=None):
    """The refinement loss of include/giga_hip.h (the reference forms it at generation.py:488-511) from the gathered corners
    (F,3,3) and the weights eps (F,3), planes of ONE scene in the dtype of the corners:
        q = sum_i eps_i v_i,  n = c / (|c| + 1e-10) with c = (v1 - v0) x (v2 - v1),  t = -g / (|g| + 1e-10) with g = d sigma(f(q)) / dq,
        loss = mean (sigma - threshold)^2 + 0.01 mean |n - t|^2.
    g stays in the autograd graph, so the loss differentiates through it.  Returns (loss, target term, normal term, q)."""
    v0, v1, v2 = corners[:, 0], corners[:, 1], corners[:, 2]
    q = eps[:, 0:1] * v0 + eps[:, 1:2] * v1 + eps[:, 2:3] * v2
    sigma = torch.sigmoid(logits(sd, planes, q[None], pre))[0]
    (g,) = torch.autograd.grad(sigma.sum(), q, create_graph=True)
    n, t = _unit(torch.cross(v1 - v0, v2 - v1, dim=1)), _unit(-g)
    target = ((sigma - threshold) ** 2).mean()
    normal = ((n - t) ** 2).sum(dim=1).mean()
    return target + 0.01 * normal, target, normal, q


def refine_loss(sd, planes, v, faces, eps, threshold=0.5, pre=None):
    """`corner_loss` for vertices v (V,3) (requires grad) and faces (F,3) long."""
    return corner_loss(sd, planes, v[faces], eps, threshold, pre)


def loss_grad(sd, planes, v, faces, eps, threshold=0.5, dtype=torch.float64, pre=None):
    """d loss / d v (V,3) by autograd, plus (loss_target, loss_normal, face_point), all detached, in `dtype`."""
    pl = cast_planes(planes, dtype)
    vv = v.detach().to(dtype).clone().requires_grad_(True)
    loss, lt, ln, q = refine_loss(sd, pl, vv, faces.long(), eps.detach().to(dtype), threshold, pre)
    (g,) = torch.autograd.grad(loss, vv)
    return g, lt.detach(), ln.detach(), q.detach()


def face_loss_grad(sd, planes, v, faces, eps, threshold=0.5, dtype=torch.float64):
    """d loss / d (corner i of face f), (F,3,3): autograd with the gathered face vertices as the leaf."""
    pl = cast_planes(planes, dtype)
    fv = v.detach().to(dtype)[faces.long()].clone().requires_grad_(True)
    loss = corner_loss(sd, pl, fv, eps.detach().to(dtype), threshold)[0]
    (g,) = torch.autograd.grad(loss, fv)
    return g


def kinked(pre, p):
    """tests/test_gpu_point_grad.py's `_excluded` for points p (B,N,3): a ReLU input of the float64 decoder within 1e-5 (relative
    to its layer's max) of zero, or an unclamped sample coordinate within 1e-4 px of a cell edge -- on ANY axis, hence on both
    axes of every cross term of the Hessian."""
    bad = torch.zeros(p.shape[:2], dtype=torch.bool)
    for t in pre:
        m = t.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1e-30)
        bad |= ((t.abs() / m) < 1e-5).any(dim=-1)
    v = p.double() / (1 + 10e-6) + 0.5
    fx = v * 39
    bad |= (((fx - fx.round()).abs() < 1e-4) & (v > -1e-6) & (v < 1 + 1e-6)).any(dim=-1)
    return bad
