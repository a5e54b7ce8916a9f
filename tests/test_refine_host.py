"""CPU tests of the mesh refinement (giga_amd.refine, csrc/giga_refine.hip, giga_decoder_point_hess): the float64 restatement
of the reference's loss (tests/refine_ref.py) against the oracle's sampler, the closed-form face gradient and the RMSprop step
(tests/refine_emu.py) against autograd and torch.optim, the C ABI's argument checks and the constructor's behaviour."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, synth
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refine_emu  # noqa: E402
import refine_ref  # noqa: E402


@pytest.fixture(scope="module")
def planes(sd7):
    return O.encoder_forward(sd7, torch.from_numpy(synth.tsdf_batch(3, 1, realistic=True)))


def _points(n, seed):
    """Inside the cube, plus clamped points (outside it) at every 8th place."""
    p = synth.query_points(seed, 1, n, stream=7, half_width=0.5).copy()
    out = synth.query_points(seed, 1, n, stream=8, half_width=0.8)
    p[:, ::8] = out[:, ::8]
    return torch.from_numpy(p).double()


def test_restated_sampler_equals_the_oracle_in_value_and_first_derivative(planes):
    pl = refine_ref.cast_planes(planes)
    p = _points(512, 5)
    w = torch.randn(1, 512, 96, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    pa, pb = p.clone().requires_grad_(True), p.clone().requires_grad_(True)
    a, b = refine_ref.sample_features(pa, pl), O.sample_features(pb, pl)
    assert a.shape == b.shape == (1, 512, 96)
    assert (a - b).abs().max().item() <= 1e-12 * b.abs().max().item()
    (ga,), (gb,) = torch.autograd.grad((a * w).sum(), pa), torch.autograd.grad((b * w).sum(), pb)
    assert (ga - gb).abs().max().item() <= 1e-12 * gb.abs().max().item()


def test_hessian_diagonal_is_zero_and_the_cross_terms_are_the_plane_formula(sd7, planes):
    """Away from cell edges the autograd Hessian of the logit has an exactly zero diagonal, is symmetric, and vanishes on a
    clamped axis; its off-diagonal entries are s_u s_v <dc, f00 - f01 - f10 + f11> per plane."""
    p = _points(256, 6)
    pre = []
    f, g, H = refine_ref.point_hess(sd7, planes, p, pre)
    keep = ~refine_ref.kinked(pre, p)[0]
    assert keep.float().mean().item() > 0.9
    H = H[0][keep]
    assert torch.equal(torch.diagonal(H, dim1=-2, dim2=-1), torch.zeros(H.shape[0], 3, dtype=torch.float64))
    assert (H - H.transpose(-1, -2)).abs().max().item() <= 1e-9 * H.abs().max().item()
    v = p[0][keep] / (1 + 10e-6) + 0.5
    clamped = (v >= 1) | (v < 0)
    assert clamped.any()
    for ax in range(3):
        assert H[clamped[:, ax]][:, ax, :].abs().max().item() == 0.0 and H[clamped[:, ax]][:, :, ax].abs().max().item() == 0.0
    # the plane formula, with dc from one more autograd call
    pl = refine_ref.cast_planes(planes)
    q = p.clone()
    c = refine_ref.sample_features(q, pl).detach().requires_grad_(True)
    (dc,) = torch.autograd.grad(refine_ref.pgrad_ref.mlp64(sd7, refine_ref.HEAD, q, c).sum(), c)
    s = 39 / (1 + 10e-6)
    vv = q[0] / (1 + 10e-6) + 0.5
    mask = ((vv < 1) & (vv >= 0)).double() * s
    fx = torch.where(vv >= 1, torch.full_like(vv, 1 - 10e-6), vv).clamp_min(0) * 39
    i0 = fx.floor().clamp(0, 38).long()
    for k, (name, (a0, a1), (r, cidx)) in enumerate(zip(O.PLANES, ((0, 2), (0, 1), (1, 2)), ((0, 2), (0, 1), (1, 2)))):
        P = pl[name][0]                                                   # (32, R, R), indexed [ch, iy(a1), ix(a0)]
        x0, y0 = i0[:, a0], i0[:, a1]
        cross = P[:, y0, x0] - P[:, y0, x0 + 1] - P[:, y0 + 1, x0] + P[:, y0 + 1, x0 + 1]      # (32, N)
        h = mask[:, a0] * mask[:, a1] * (dc[0, :, 32 * k:32 * k + 32].T * cross).sum(0)
        ref = refine_ref.point_hess(sd7, planes, p)[2][0][:, r, cidx]
        assert (h[keep] - ref[keep]).abs().max().item() <= 1e-9 * max(ref.abs().max().item(), 1e-30), name


@pytest.mark.parametrize("n_faces, seed", [(4, 1), (33, 2), (129, 3)])
def test_face_gradient_emulation_equals_autograd_of_the_restated_loss(sd7, planes, n_faces, seed):
    v, faces = refine_emu.hand_mesh(n_faces, seed)
    eps = refine_emu.dirichlet(n_faces, seed)
    deg = refine_emu.degenerate(v, faces)
    assert deg[-1] and not deg[:-1].any()                                 # the zero-area face
    valence = np.bincount(faces.reshape(-1), minlength=len(v))
    assert valence[-1] == 0                                               # the unreferenced vertex
    if n_faces >= 129:
        assert valence.max() >= 40
    tv, tf, te = torch.from_numpy(v), torch.from_numpy(faces), torch.from_numpy(eps)
    g_ref, lt, ln, q = refine_ref.loss_grad(sd7, planes, tv, tf, te, 0.5)
    f, df, H = refine_ref.point_hess(sd7, planes, q[None])
    hess = torch.stack((H[0, :, 0, 1], H[0, :, 0, 2], H[0, :, 1, 2]), dim=-1)
    loss, fg = refine_emu.face_grad(v, faces, eps, f[0].numpy(), df[0].numpy(), hess.numpy(), 0.5)
    assert abs(loss[:, 0].mean() - lt.item()) <= 1e-12 and abs(loss[:, 1].mean() - ln.item()) <= 1e-12
    g = refine_emu.vertex_grad(fg, faces, len(v))
    touched = np.zeros(len(v), bool)
    touched[faces[deg].reshape(-1)] = True
    scale = np.abs(g_ref.numpy()[~touched]).max()                         # (the zero-area face's 1 / eps gradient would hide the rest)
    assert np.allclose(g, g_ref.numpy(), rtol=1e-9, atol=1e-9 * scale)
    assert np.abs(g_ref.numpy()[touched]).max() > 1e3 * scale             # ... and it is there: c / (|c| + 1e-10) at c = 0
    assert (g[-1] == 0).all() and (g_ref.numpy()[-1] == 0).all()
    # the CSR corner list sums the same corners
    order, off = refine_emu.csr(faces, len(v))
    flat = fg.reshape(-1, 3)
    for vert in (0, 1, len(v) - 1):
        assert np.allclose(flat[order[off[vert]:off[vert + 1]]].sum(0), g[vert], rtol=1e-12, atol=1e-12 * scale)
        assert (faces.reshape(-1)[order[off[vert]:off[vert + 1]]] == vert).all()


def test_rmsprop_emulation_equals_torch_optim_over_three_steps():
    gen = torch.Generator().manual_seed(4)
    v0 = torch.randn(50, 3, dtype=torch.float64, generator=gen)
    grads = [torch.randn(50, 3, dtype=torch.float64, generator=gen) * 10.0 ** (k - 1) for k in range(3)]
    grads[1][7] = 0.0                                                     # a zero gradient moves nothing
    param = torch.nn.Parameter(v0.clone())
    opt = torch.optim.RMSprop([param], lr=1e-4)
    v, sq = v0.numpy().copy(), np.zeros((50, 3))
    for g in grads:
        opt.zero_grad()
        param.grad = g.clone()
        opt.step()
        before = v.copy()
        v, sq = refine_emu.rmsprop(v, sq, g.numpy())
        assert np.abs(v - param.detach().numpy()).max() <= 1e-15
        assert np.abs(v - before).max() <= refine_emu.LR / np.sqrt(1 - refine_emu.ALPHA) + 1e-12
    assert (v[7] != v0.numpy()[7]).all() and np.abs(sq - opt.state[param]["square_avg"].numpy()).max() <= 1e-12 * sq.max()


# ---- C ABI -------------------------------------------------------------------------------------------------------------
_BUF = (ctypes.c_float * 64)()
_A = ctypes.cast(_BUF, ctypes.c_void_p)                  # never dereferenced: every check precedes the first launch
_NUL = ctypes.c_void_p(0)


def _p(on):
    return _A if on else _NUL


def test_refinement_symbols_are_exported_and_declared():
    L = _capi.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "giga_hip.h")).read()
    for name in ("giga_decoder_point_hess", "giga_refine_face_points", "giga_refine_face_grad", "giga_refine_vertex_step"):
        assert hasattr(L, name) and name in _capi.EXPORTS and ("int %s(" % name) in hdr, name
    assert "#define GIGA_REFINE_MAX_FACES 0x%08X" % _capi.REFINE_MAX_FACES in hdr
    assert L.giga_abi_version() == 3


def _hess(planes=True, p=True, blob=True, bwd=True, logit=True, dp=True, hess=True, B=1, N=4):
    return _capi.lib().giga_decoder_point_hess(_p(planes), _p(p), _p(blob), _p(bwd), _p(logit), _p(dp), _p(hess), B, N, _NUL)


@pytest.mark.parametrize("kwargs, code", [
    (dict(planes=False), -1), (dict(p=False), -1), (dict(blob=False), -1), (dict(bwd=False), -1),
    (dict(logit=False), -1), (dict(dp=False), -1), (dict(hess=False), -1),
    (dict(B=0), -1), (dict(N=0), -1), (dict(B=-2), -1), (dict(N=-1), -1),
    (dict(B=_capi.MAX_SCENES + 1), -7),
    (dict(B=2048, N=1 << 20), -1),                        # B * N = 2^31, as giga_decoder_point_grad
])
def test_point_hess_rejects_invalid_arguments_without_a_device(kwargs, code):
    assert _hess(**kwargs) == code


def test_refine_entry_points_reject_invalid_arguments_without_a_device():
    L = _capi.lib()
    big = _capi.REFINE_MAX_FACES + 1

    def points(v=True, f=True, eps=True, q=True, V=4, F=2, step=0):
        return L.giga_refine_face_points(_p(v), _p(f), _NUL, _p(eps), _p(q), V, F, 7, step, _NUL)

    assert points(F=0) == 0
    assert points(v=False) == -1 and points(f=False) == -1 and points(V=-1) == -1 and points(F=-1) == -1
    assert points(step=-1) == -1 and points(F=big) == -1 and points(V=big) == -1
    assert points(eps=False) == -6 and points(q=False) == -6

    def grad(v=True, f=True, eps=True, logit=True, dp=True, hess=True, loss=True, out=True, V=4, F=2, tau=0.5):
        return L.giga_refine_face_grad(_p(v), _p(f), _p(eps), _p(logit), _p(dp), _p(hess), tau, _p(loss), _p(out), V, F, _NUL)

    assert grad(F=0) == 0
    for name in ("v", "f", "eps", "logit", "dp", "hess"):
        assert grad(**{name: False}) == -1, name
    assert grad(tau=0.0) == -1 and grad(tau=1.0) == -1 and grad(tau=float("nan")) == -1
    assert grad(V=-1) == -1 and grad(F=big) == -1
    assert grad(loss=False) == -6 and grad(out=False) == -6

    def step(fg=True, order=True, off=True, v=True, sq=True, g=True, V=4, F=2):
        return L.giga_refine_vertex_step(_p(fg), _p(order), _p(off), _p(v), _p(sq), _p(g), V, F, _NUL)

    assert step(V=0) == 0
    assert step(fg=False) == -1 and step(order=False) == -1 and step(off=False) == -1 and step(v=False) == -1
    assert step(sq=False) == -1 and step(V=-1) == -1 and step(F=-1) == -1 and step(V=big) == -1
    assert step(g=False) == -6


# ---- Python surface ------------------------------------------------------------------------------------------------------
def test_generator_refinement_arguments():
    from giga_amd.generation import Generator3D
    with pytest.raises(NotImplementedError, match="runs only on a HIP device"):
        Generator3D(None, device=torch.device("cpu"), refinement_step=1)
    gen = Generator3D(None, refinement_step=3, refine_seed=5)             # the default device is the HIP device
    assert gen.refinement_step == 3 and gen.refine_seed == 5 and gen.mesh_options["refinement_step"] == 3
    assert Generator3D(None, device=torch.device("cuda:0"), refinement_step=2).refinement_step == 2
    assert Generator3D(None, device=torch.device("cpu")).refinement_step == 0
    with pytest.raises(NotImplementedError):
        Generator3D(None, refinement_step=1, simplify_nfaces=100)
    with pytest.raises(NotImplementedError):
        Generator3D(None, refinement_step=-1)
    assert hasattr(gen, "refine_mesh")


def test_refiner_and_point_hess_on_cpu_tensors_raise_giga_error():
    from giga_amd.convonet import decoder_point_hess
    from giga_amd.refine import MeshRefiner
    z = torch.zeros(3, 1, 40, 40, 32)
    with pytest.raises(_capi.GigaHipError):
        decoder_point_hess(z, torch.zeros(1, 4, 3), torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(_capi.GigaHipError):
        MeshRefiner(None, z, np.zeros((3, 3), np.float32), np.array([[0, 1, 2]]))
