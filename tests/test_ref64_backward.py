"""CPU checks of the float64 training reference of tests/ref64.py (train_grads): it agrees with fp32 oracle autograd and with
goldens G4 / G8, its census finds the ties it should, and the per-tensor tolerance of
tests/test_gpu_backward_envelope.py (ref64.TOL_BWD) rejects three realistic backward bugs by at least 4x: the tie-all
max-pool rule, a ReLU backward that passes gradient at z = 0, and one U-Net layer's data gradient with bf16 operands."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from giga_amd import synth
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402
import test_gpu_backward_envelope as E  # noqa: E402  (its case list and batches; its tests need a GPU and skip here)

_max_pool2d, _relu, _conv2d = F.max_pool2d, F.relu, F.conv2d


def _g4_batch(g4):
    B, M, s0 = int(g4["B"]), int(g4["M"]), int(g4["first_scene"])
    x = torch.from_numpy(synth.tsdf_batch(s0, B))
    pos = torch.from_numpy(synth.query_points(s0, B, 1, stream=2))
    pos_occ = torch.from_numpy(synth.query_points(s0, B, M, stream=3))
    y = tuple(torch.from_numpy(a) for a in synth.train_labels(s0, B, M))
    return x, pos, pos_occ, y


def _worst(got, ref):
    return max((ref64.grad_err(got[k], ref[k]), k) for k in ref)


@pytest.mark.parametrize("detach", [False, True])
def test_train_grads_match_fp32_oracle_and_goldens(golden, sd7, detach):
    """Float64 gradients against fp32 autograd through the oracle (measured worst 7.7e-5 of the tensor's max, the occupancy
    head's blocks.1.fc_0: the oracle samples the planes in fp32; the same chain in fp32 is within 7e-6), against the
    reference-generated per-tensor gradient norms of G4 (G8 with detach_tsdf; measured 2.4e-6 relative) and against G4's
    float64-summed conv_in weight gradient (measured 1.7e-6 of its max)."""
    g4 = golden("g4_train_step.npz")
    x, pos, pos_occ, y = _g4_batch(g4)
    parts, g64 = ref64.train_grads(sd7, x, pos, pos_occ, y, detach_tsdf=detach)
    _, g32 = ref64.train_grads(sd7, x, pos, pos_occ, y, detach_tsdf=detach, dtype=torch.float32)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd7.items()}
    loss, d = O.train_loss(O.train_select(O.model_forward(sdg, x, pos, p_tsdf=pos_occ, detach_tsdf=detach)), y)
    loss.backward()
    assert set(g64) == set(sd7) and all(v.dtype == torch.float64 for v in g64.values())
    assert _worst(g32, g64)[0] <= 2e-5, _worst(g32, g64)
    assert _worst({k: v.grad for k, v in sdg.items()}, g64)[0] <= 1.5e-4, _worst({k: v.grad for k, v in sdg.items()}, g64)
    for k, v in d.items():
        assert abs(parts[k] - v.item()) <= 1e-6 * max(1.0, abs(parts[k])), k
    g = golden("g8_detach.npz") if detach else g4
    for n, r in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        assert abs(g64[n].norm().item() - r) <= 1e-5 * max(r, 1e-6), (n, g64[n].norm().item(), r)
    if not detach:
        ref = g4["grad_conv_in_w_f64"]
        assert np.abs(g64["encoder.conv_in.weight"].numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
        for k in ("loss_qual", "loss_rot", "loss_width", "loss_occ", "loss_all"):
            assert abs(parts[k] - float(g4[k])) <= 1e-5 * max(1.0, abs(float(g4[k]))), k


def test_smooth_objective_and_head_subsets(sd7):
    """The smooth objective's gradient equals the sum of the per-head ones, and the head subsets of giga_aff / giga_geo
    return exactly their model's parameters with the encoder gradient of their heads alone."""
    x = torch.from_numpy(synth.tsdf_batch(3, 2))
    pos = torch.from_numpy(synth.query_points(3, 2, 3, stream=2))
    po = torch.from_numpy(synth.query_points(3, 2, 100, stream=3))
    R = ref64.smooth_objective(2, 3, 100)
    _, full = ref64.train_grads(sd7, x, pos, po, objective=R)
    _, aff = ref64.train_grads(sd7, x, pos, po, heads=ref64.HEADS[:3], objective={h: R[h] for h in ref64.HEADS[:3]})
    _, geo = ref64.train_grads(sd7, x, pos, po, heads=ref64.HEADS[3:], objective={"decoder_tsdf": R["decoder_tsdf"]})
    assert not any(k.startswith("decoder_tsdf.") for k in aff) and all(k.startswith(("encoder.", "decoder_tsdf.")) for k in geo)
    for k, v in full.items():
        want = (aff[k] if k in aff else 0) + (geo[k] if k in geo else 0)
        assert (v - want).abs().max().item() <= 1e-12 * max(1.0, v.abs().max().item()), k


def test_census_counts_ties_and_zeros():
    """Exact positive ties are plentiful on 'structured' scenes (constant regions) and absent on uniform noise; the empty
    adversarial scene with bias-free weights has exactly-zero ReLU inputs."""
    he7, nb = ref64.weight_family("he-7"), ref64.weight_family("nobias")
    st = ref64.census(he7, torch.from_numpy(ref64.input_family("structured", 1)), heads=())
    un = ref64.census(he7, torch.from_numpy(ref64.input_family("uniform", 1)), heads=())
    em = ref64.census(nb, torch.from_numpy(ref64.input_family("adversarial", 1)), heads=())
    assert st["pool_ties"] > 1000 and un["pool_ties"] == 0, (st, un)
    assert em["relu_zero"] > 0, em


# ---- sensitivity: what TOL_BWD rejects -----------------------------------------------------------------------------
class _TieAllPool(torch.autograd.Function):
    """The kernels' former pool backward: every element equal to its window's maximum receives the window's gradient."""

    @staticmethod
    def forward(ctx, s):
        q = _max_pool2d(s, 2, 2)
        ctx.save_for_backward(s, q)
        return q

    @staticmethod
    def backward(ctx, g):
        s, q = ctx.saved_tensors
        up = lambda t: t.repeat_interleave(2, -1).repeat_interleave(2, -2)  # noqa: E731
        return (s == up(q)).to(g.dtype) * up(g)


class _ReluGe(torch.autograd.Function):
    """ReLU whose backward passes the gradient at z = 0 too ('>=' for '>')."""

    @staticmethod
    def forward(ctx, z):
        ctx.save_for_backward(z)
        return _relu(z)

    @staticmethod
    def backward(ctx, g):
        (z,) = ctx.saved_tensors
        return g * (z >= 0).to(g.dtype)


class _Bf16Dgrad(torch.autograd.Function):
    """conv2d (3x3, padding 1) whose data gradient takes bf16-rounded operands (dY and W), fp64 accumulation."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _conv2d(x, w, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        bf = lambda t: t.bfloat16().to(t.dtype)  # noqa: E731
        dx = torch.nn.grad.conv2d_input(x.shape, bf(w), bf(g), padding=1)
        return dx, torch.nn.grad.conv2d_weight(x, w.shape, g, padding=1), g.sum((0, 2, 3))


UNET_CONVS = ("down_convs.0.conv1", "down_convs.0.conv2", "down_convs.1.conv1", "down_convs.1.conv2", "down_convs.2.conv1",
              "down_convs.2.conv2", "up_convs.0.conv1", "up_convs.0.conv2", "up_convs.1.conv1", "up_convs.1.conv2")


def _bf16_dgrad_at(layer):
    """F.conv2d for oracle.unet_forward whose `layer`-th 3x3 convolution (of 11 calls per plane) has a bf16 data gradient."""
    calls = [0]

    def conv(x, w, b=None, *a, **k):
        i = calls[0]
        calls[0] += 1
        return _Bf16Dgrad.apply(x, w, b) if i % 11 == layer else _conv2d(x, w, b, *a, **k)
    return conv


def _mutant_err(case, **fns):
    x, pos, pos_occ, y = E.batch(case)
    kw = dict(heads=E.HEADS_OF[case[0]], objective=E.objective(case))
    sd = E.state_dict(case)
    _, ref = ref64.train_grads(sd, x, pos, pos_occ, y, **kw)
    with ref64.patched_functional(**fns):
        _, bad = ref64.train_grads(sd, x, pos, pos_occ, y, **kw)
    return _worst(bad, ref)


@pytest.mark.parametrize("wfam", ["he-7", "spread", "nobias"])
def test_tolerance_rejects_the_tie_all_pool_rule(wfam):
    err = _mutant_err(("giga", wfam, "structured", 3, 1, 300, "loss"), max_pool2d=lambda s, *a, **k: _TieAllPool.apply(s))
    assert err[0] >= 4 * ref64.TOL_BWD, err


@pytest.mark.parametrize("obj", ["loss", "smooth"])
def test_tolerance_rejects_a_relu_backward_at_zero(obj):
    """Bias-free weights on the empty and single-voxel scenes: conv_in's pre-activations are exactly 0 over empty space."""
    err = _mutant_err(("giga", "nobias", "adversarial", 3, 1, 300, obj), relu=lambda z, *a, **k: _ReluGe.apply(z))
    assert err[0] >= 4 * ref64.TOL_BWD, err


@pytest.mark.parametrize("layer", range(10), ids=UNET_CONVS)
def test_tolerance_rejects_one_bf16_data_gradient(layer):
    err = _mutant_err(("giga", "he-7", "uniform", 3, 1, 300, "loss"), conv2d=_bf16_dgrad_at(layer))
    assert err[0] >= 4 * ref64.TOL_BWD, (UNET_CONVS[layer], err)
