"""CPU tests of the query-point gradients: the C ABI entry point giga_decoder_point_grad exists and rejects every invalid
argument before touching a device, grad_refine fails loudly on CPU tensors, and the float64 restatement of tests/pgrad_ref.py
is pinned against the live reference (marked `reference`)."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, networks, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pgrad_ref  # noqa: E402


def _call(head_mask=1, dq=True, drot=True, dwidth=True, dtsdf=True, dp=True, B=1, N=4, flags=0):
    L = _capi.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    nul = ctypes.c_void_p(0)
    return L.giga_decoder_point_grad(a, a, a, a, head_mask, a if dq else nul, a if drot else nul, a if dwidth else nul,
                                     a if dtsdf else nul, a if dp else nul, nul, nul, nul, nul, B, N, flags, nul)


def test_point_grad_is_exported():
    L = _capi.lib()
    assert hasattr(L, "giga_decoder_point_grad")
    assert "giga_decoder_point_grad" in _capi.EXPORTS
    assert L.giga_abi_version() == 3


@pytest.mark.parametrize("kwargs, code", [
    (dict(head_mask=0), -1),
    (dict(head_mask=16), -1),
    (dict(head_mask=1 | 32), -1),
    (dict(head_mask=-1), -1),
    (dict(head_mask=1, dq=False), -6),
    (dict(head_mask=2, drot=False), -6),
    (dict(head_mask=4, dwidth=False), -6),
    (dict(head_mask=8, dtsdf=False), -6),
    (dict(head_mask=7, dwidth=False), -6),
    (dict(dp=False), -1),
    (dict(B=0), -1),
    (dict(N=0), -1),
    (dict(B=-2), -1),
    (dict(N=-1), -1),
    (dict(B=_capi.MAX_SCENES + 1), -7),
    (dict(B=2048, N=1 << 20), -1),                # B * N = 2^31: beyond the kernel's point index
    (dict(flags=_capi.FOLD_FINAL), -5),           # folded planes have no transposed fc_c images
])
def test_point_grad_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _call(**kwargs) == code


def test_grad_refine_on_cpu_tensors_raises_giga_error():
    net = networks.get_network("giga")
    x = torch.zeros(1, 40, 40, 40)
    pos = torch.zeros(1, 4, 3)
    with pytest.raises(_capi.GigaHipError):
        net.grad_refine(x, pos)


def test_estimate_normals_on_cpu_planes_raises_giga_error():
    from giga_amd.generation import Generator3D
    from giga_amd.convonet import PlaneDict
    net = networks.get_network("giga")
    c = PlaneDict((k, torch.zeros(1, 32, 40, 40)) for k in ("xz", "xy", "yz"))
    with pytest.raises(_capi.GigaHipError):
        Generator3D(net, device=torch.device("cpu")).estimate_normals(np.zeros((3, 3), np.float32), c)


# ---- the restatement against the live reference ----------------------------------------------------------------
def _reference_or_skip():
    from oracle import ref_bootstrap
    if not ref_bootstrap.reference_available():
        pytest.skip("reference not present (build container only)")
    return ref_bootstrap


def test_point_grad_restatement_matches_finite_differences(sd7):
    """The restatement itself: central differences in float64 (a point away from cell edges and clamps)."""
    from oracle import giga_oracle as O
    x = torch.from_numpy(synth.tsdf_batch(3, 1))
    planes = O.encoder_forward(sd7, x)
    p = torch.tensor([[[0.113, -0.207, 0.031]]], dtype=torch.float64)
    dq = {"decoder_qual": torch.ones(1, 1, dtype=torch.float64), "decoder_width": torch.full((1, 1), 0.5, dtype=torch.float64)}
    g = pgrad_ref.point_grad(sd7, planes, p, dq)
    pl = {k: v.double() for k, v in planes.items()}

    def f(q):
        out = pgrad_ref.head_outputs(sd7, pl, q, list(dq))
        return sum((out[h] * dq[h]).sum() for h in dq).item()

    for j in range(3):
        e = torch.zeros_like(p)
        e[..., j] = 1e-6
        fd = (f(p + e) - f(p - e)) / 2e-6
        assert abs(fd - g[0, 0, j].item()) <= 1e-5 * max(1.0, abs(fd)), (j, fd, g[0, 0, j].item())


@pytest.mark.reference
@pytest.mark.parametrize("lr, num_step", [(1e-6, 1), (1e-3, 3)])
def test_grad_refine_restatement_matches_reference(sd7, lr, num_step):
    rb = _reference_or_skip()
    ref = rb.load_reference_giga(sd7)
    x = torch.from_numpy(synth.tsdf_batch(5, 2, realistic=True))
    pos = torch.from_numpy(synth.query_points(5, 2, 16, stream=4, half_width=0.45))
    q_ref, p_ref, r_ref, w_ref = ref.grad_refine(x, pos, lr=lr, num_step=num_step)
    q, p, r, w = pgrad_ref.grad_refine(sd7, x, pos, lr=lr, num_step=num_step)
    assert (p - p_ref.detach().double()).abs().max().item() < 1e-6
    assert (p - pos.double()).abs().max().item() > 0.0 or lr < 1e-5      # the larger step moves the points
    for a, b in ((q, q_ref), (r, r_ref), (w, w_ref)):
        assert (a - b.detach()).abs().max().item() < 1e-4


@pytest.mark.reference
def test_estimate_normals_restatement_matches_reference(sd7):
    rb = _reference_or_skip()
    ref = rb.load_reference_giga(sd7)
    x = torch.from_numpy(synth.tsdf_batch(6, 1, realistic=True))
    v = synth.query_points(6, 1, 64, stream=5, half_width=0.45)[0]
    c = ref.encode_inputs(x)
    try:                                                 # the reference's own generator, if it imports with the stubs
        from vgn.ConvONets.conv_onet.generation import Generator3D as RefGen  # type: ignore
        gen = RefGen(ref, points_batch_size=100000, device=torch.device("cpu"))
        vi = torch.from_numpy(v)[None].requires_grad_()
        occ = ref.decode_occ(vi, c).logits
        occ.sum().backward()
        n_ref = (-vi.grad / torch.norm(vi.grad, dim=-1, keepdim=True))[0].numpy()
        assert gen.model is ref
    except ImportError:
        vi = torch.from_numpy(v)[None].requires_grad_()
        occ = ref.decoder_tsdf(vi, c)
        (g,) = torch.autograd.grad(occ.sum(), vi)
        n_ref = (-g / torch.norm(g, dim=-1, keepdim=True))[0].numpy()
    from oracle import giga_oracle as O
    n = pgrad_ref.estimate_normals(sd7, O.encoder_forward(sd7, x), v)
    cos = (n * n_ref).sum(-1)
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-9
    assert cos.min() > 0.9999, cos.min()
