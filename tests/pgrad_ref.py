"""Test-side restatement of the query-point gradients (float64 torch autograd through oracle.giga_oracle's sampling):
the decoder heads' d/dp, ConvolutionalOccupancyNetwork.grad_refine (reference models/__init__.py:136-164) and
Generator3D.estimate_normals (conv_onet/generation.py:430-455).  Test infrastructure only."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import giga_oracle as O

HEADS = ("decoder_qual", "decoder_rot", "decoder_width", "decoder_tsdf")


def mlp64(sd, head, p, c, pre=None):
    """oracle.decoder_mlp in the dtype of its inputs (the oracle's casts p to fp32); `pre` collects every ReLU input."""
    def lin(name, t):
        return F.linear(t, sd[f"{head}.{name}.weight"].to(t.dtype), sd[f"{head}.{name}.bias"].to(t.dtype))

    def relu(t):
        if pre is not None:
            pre.append(t.detach())
        return F.relu(t)

    net = lin("fc_p", p)
    for i in range(5):
        net = net + lin(f"fc_c.{i}", c)
        h = lin(f"blocks.{i}.fc_0", relu(net))
        net = net + lin(f"blocks.{i}.fc_1", relu(h))
    return lin("fc_out", relu(net)).squeeze(-1)


def head_outputs(sd, planes, p, heads, pre=None):
    """Post-epilogue outputs (models/__init__.py:111-124) of `heads` at p, float64."""
    c = O.sample_features(p, planes)
    out = {}
    for h in heads:
        z = mlp64(sd, h, p, c, pre)
        out[h] = torch.sigmoid(z) if h == "decoder_qual" else F.normalize(z, dim=2) if h == "decoder_rot" else z
    return out


def point_grad(sd, planes, p, douts, pre=None, dtype=torch.float64):
    """d/dp sum_h <douts[h], head_h(p)> in float64 (or `dtype`); planes {'xz','xy','yz'}: (B,32,40,40)."""
    pl = {k: v.detach().to(dtype) for k, v in planes.items()}
    p64 = p.detach().to(dtype).clone().requires_grad_(True)
    out = head_outputs(sd, pl, p64, list(douts), pre)
    s = sum((out[h] * douts[h].to(dtype)).sum() for h in douts)
    (g,) = torch.autograd.grad(s, p64)
    return g


def grad_refine(sd, x, pos, bound_value=0.0125, lr=1e-6, num_step=1):
    """models/__init__.py:136-164: SGD(lr) on -qual.sum() w.r.t. the positions, float64, planes of the oracle encoder.
    Returns (qual, pos_refined, rot, width), outputs from the fp32 oracle at the refined positions."""
    planes = O.encoder_forward(sd, x.float())
    pos_tmp = pos.double().clone()
    for _ in range(num_step):
        dq = point_grad(sd, planes, pos_tmp, {"decoder_qual": torch.ones(pos.shape[:-1], dtype=torch.float64)})
        pos_tmp = pos_tmp + lr * dq
    pos64 = pos.double()
    pos_tmp = torch.maximum(torch.minimum(pos_tmp, pos64 + bound_value), pos64 - bound_value)
    qual, rot, width = O.decode(sd, pos_tmp.float(), planes)
    return qual, pos_tmp, rot, width


def estimate_normals(sd, planes, vertices):
    """generation.py:430-455: -grad_p(occupancy logit) / |.|, (N,3) numpy, float64 arithmetic."""
    v = torch.as_tensor(np.asarray(vertices), dtype=torch.float64)[None]
    g = point_grad(sd, planes, v, {"decoder_tsdf": torch.ones(v.shape[:-1], dtype=torch.float64)})
    n = -g
    return (n / torch.norm(n, dim=-1, keepdim=True))[0].numpy()
