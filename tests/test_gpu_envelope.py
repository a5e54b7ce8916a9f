"""The forward path held to a float64 reference (tests/ref64.py) away from the one operating point the parity tests use:
five weight families x four input families at 3 and 33 scenes in every precision / U-Net form, exact power-of-two
homogeneity of the fp32 kernels, and the input-scale window of the f16-class modes.

Errors are range-relative: max |got - ref| / (max ref - min ref), per scene and output (ref64.range_err).  The fp32-class
tolerances (ref64.TOL) are tied to a bug they must catch by tests/test_ref64.py::test_tolerance_rejects_one_layer_in_f16."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import networks, synth
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("qual", "rot", "width", "tsdf")
HEAD_OF = dict(zip(OUTS, ref64.HEADS))
# (label, precision, U-Net kernel, persistent_unet)
MODES = (("fp32", "fp32", "auto", False), ("fp32-direct", "fp32", "direct", False),
         ("fp32-persistent", "fp32", "auto", True), ("fp32-layers", "fp32", "auto", "layers"),
         ("fp16x3", "fp16x3", "auto", False), ("fp16", "fp16", "auto", False), ("fp16x3+fp16", "fp16x3+fp16", "auto", False))
FP32_FORMS = [m for m in MODES if m[1] == "fp32"]
# Plain f16 operands (the throughput modes).  'fp16' keeps today's envelope (tests/test_gpu_parity.py::test_model_forward_g2,
# absolute) on the builder's weights with U[0,1) inputs: 1e-2 on sigmoid(qual), 1.5e-2 on the unit quaternion, 2e-2 on raw
# width / occupancy logits and on the planes (measured here: 9.0e-4, 1.14e-2, 3.9e-3, 3.5e-3, 4.3e-3).
F16_ABS = {"planes": 2e-2, "qual": 1e-2, "rot": 1.5e-2, "width": 2e-2, "tsdf": 2e-2}
# ... and range-relative on every other family, and for the plain-f16 lattice decoder of 'fp16x3+fp16' (its quaternions by
# ref64.rot_err): measured worst 4.6e-3 ('spread' width), bound 2x that, rounded up.
F16_REL = 1e-2
# 'spread' drives the heads' hidden activations to 2.6e5 (float64), past the f16 range: the f16-class modes must return NaN /
# inf there, and every finite entry must still meet its tolerance (ref64.finite_err).  (Before the qual epilogue kept an
# infinite logit as NaN, plain fp16 returned sigmoid(+-inf) there: a finite qual of 0 or 1, the wrong one for some points.)
PAST_F16_RANGE = ("spread",)
N_POINTS = 512

_MEASURED = {}


def _record(key, err):
    _MEASURED[key] = max(_MEASURED.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    rows = sorted(_MEASURED.items())
    print("\nENVELOPE worst range-relative errors:")
    for k, v in rows:
        print("ENVELOPE", "/".join(map(str, k)), f"{v:.3e}")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_NETS = {}


def _net(fam, dev):
    if fam not in _NETS:
        n = networks.get_network("giga")
        n.load_state_dict(ref64.weight_family(fam))
        _NETS[fam] = n.to(dev).eval()
    return _NETS[fam]


def _configure(net, prec, kernel, persist):
    net.set_precision(prec)
    net.set_unet_kernel(kernel)
    net.set_persistent_unet(persist)
    return net


def _lattice(dev):
    return torch.from_numpy(synth.inference_lattice()).to(dev)


_REF = {}


def _reference(wfam, ifam, B, lattice):
    """float64 planes and head outputs of the sampled scenes (first, middle, last), cached per module."""
    key = (wfam, ifam, B, lattice)
    if key not in _REF:
        ks = sorted({0, B // 2, B - 1} | ({1, 2, 3} & set(range(B)) if ifam == "adversarial" else set()))
        sd = ref64.weight_family(wfam)
        x = torch.from_numpy(ref64.input_family(ifam, B))
        p = torch.from_numpy(synth.inference_lattice()).expand(len(ks), -1, -1) if lattice else \
            torch.from_numpy(synth.query_points(0, B, N_POINTS, stream=1, half_width=0.55))[ks]
        planes = ref64.encoder(sd, x[ks])
        raw, out = ref64.heads(sd, planes, p)
        _REF[key] = (ks, x, p, planes, out, raw["decoder_rot"])
    return _REF[key]


def _tol(label, wfam, ifam, what):
    if label.startswith("fp32"):
        return ref64.TOL["fp32"]
    if label == "fp16x3" or (label == "fp16x3+fp16" and what == "planes"):
        return ref64.TOL["fp16x3"]
    return None      # plain-f16 arithmetic: F16_REL (F16_ABS on the trusted families)


# ---- 2. family sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [3, 33])
@pytest.mark.parametrize("ifam", ref64.INPUT_FAMILIES)
@pytest.mark.parametrize("wfam", ref64.WEIGHT_FAMILIES)
@pytest.mark.parametrize("mode", MODES, ids=[m[0] for m in MODES])
def test_forward_matches_float64(dev, mode, wfam, ifam, B):
    """net(x, p, p_tsdf=p) and encode_inputs(x) against float64 on the first, middle and last scene (and all four adversarial
    scenes).  'fp16x3+fp16' runs the inference lattice (its plain-f16 lattice decoder); every other mode 512 points per
    scene, both coordinate clamps hit."""
    label, prec, kernel, persist = mode
    lattice = label == "fp16x3+fp16"
    ks, x, p, ref_planes, ref_out, ref_rot_raw = _reference(wfam, ifam, B, lattice)
    net = _configure(_net(wfam, dev), prec, kernel, persist)
    xd = x.to(dev)
    pd = _lattice(dev) if lattice else torch.from_numpy(synth.query_points(0, B, N_POINTS, stream=1, half_width=0.55)).to(dev)
    try:
        with torch.no_grad():
            planes = net.encode_inputs(xd)
            outs = dict(zip(OUTS, net(xd, pd, p_tsdf=pd)))
        torch.cuda.synchronize()
    finally:
        _configure(net, "fp32", "auto", False)
    f16class = not label.startswith("fp32")
    trusted = label == "fp16" and wfam.startswith("he-") and ifam in ("uniform", "realistic")
    fails = []
    for j, k in enumerate(ks):
        for what in ("planes",) + OUTS:
            if what == "planes":
                ref_t = torch.stack([ref_planes[key][j] for key in O.PLANES])
                g_t = torch.stack([planes[key][k].double().cpu() for key in O.PLANES])
            else:
                ref_t, g_t = ref_out[HEAD_OF[what]][j], outs[what][k].double().cpu()
            tol = _tol(label, wfam, ifam, what)
            if tol is None:
                tol = F16_REL
            if what == "rot" and lattice:
                e = ref64.rot_err(g_t, ref_t, ref_rot_raw[j], finite_only=wfam in PAST_F16_RANGE)
                if wfam in PAST_F16_RANGE:
                    e, n_bad = e
                    _record((label, wfam, ifam, what, "non-finite entries"), n_bad)
            elif f16class and wfam in PAST_F16_RANGE:
                e, n_bad = ref64.finite_err(g_t, ref_t)
                _record((label, wfam, ifam, what, "non-finite entries"), n_bad)
            else:
                e = ref64.range_err(g_t, ref_t)
            _record((label, wfam, ifam, what), e)
            ok = e <= tol
            if trusted:
                ea = (g_t - ref_t).abs().max().item() if bool(torch.isfinite(g_t).all()) else float("inf")
                _record((label, wfam, ifam, what, "abs"), ea)
                ok = ea <= F16_ABS[what]
            if not ok:
                fails.append((k, what, e))
    assert not fails, fails


# ---- 3a. exact power-of-two homogeneity of fp32 ---------------------------------------------------------------------
SCALES = (2.0 ** -8, 2.0 ** -3, 2.0 ** 3, 2.0 ** 8)


@pytest.mark.parametrize("ifam", ["adversarial", "structured"])
@pytest.mark.parametrize("mode", FP32_FORMS, ids=[m[0] for m in FP32_FORMS])
def test_fp32_encoder_is_exactly_homogeneous(dev, mode, ifam):
    """With zero biases every fp32 operation commutes exactly with a power-of-two scale (nothing here is subnormal or
    overflows), so encode_inputs(s x) == s encode_inputs(x) bit for bit.  A mismatch means an absolute constant hides in a
    kernel: a halo that is not zero, a stale bias, a clamp."""
    label, prec, kernel, persist = mode
    net = _configure(_net("nobias", dev), prec, kernel, persist)
    x = torch.from_numpy(ref64.input_family(ifam, 33)).to(dev)
    try:
        with torch.no_grad():
            base = net.encode_inputs(x)
            for s in SCALES:
                sc = net.encode_inputs(x * s)
                for key in O.PLANES:
                    assert torch.equal(sc[key], base[key] * s), (s, key)
                assert torch.equal(sc.nhwc, base.nhwc * s), s
    finally:
        _configure(net, "fp32", "auto", False)


@pytest.mark.parametrize("entry", ["generic", "lattice"])
def test_fp32_decoders_are_exactly_homogeneous(dev, entry):
    """Raw logits of every head on s * planes == s * logits, bit for bit (zero biases, zero fc_p: the heads are then
    positively homogeneous in the planes)."""
    from giga_amd import convonet
    net = _configure(_net("nobias-nofcp", dev), "fp32", "auto", False)
    g = torch.Generator().manual_seed(41)
    planes = {k: torch.randn(5, 32, 40, 40, generator=g).to(dev) for k in O.PLANES}
    p = _lattice(dev) if entry == "lattice" else torch.from_numpy(synth.query_points(3, 5, 4096, stream=1, half_width=0.6)).to(dev)
    before = dict(convonet.LATTICE_STATS)
    with torch.no_grad():
        for h in ref64.HEADS:
            dec = getattr(net, h)
            base = dec(p, planes)
            for s in SCALES:
                got = dec(p, {k: v * s for k, v in planes.items()})
                assert torch.equal(got, base * s), (h, s)
    assert convonet.LATTICE_STATS["fast" if entry == "lattice" else "generic"] > before["fast" if entry == "lattice" else "generic"]


# ---- 3b. the f16-class window ---------------------------------------------------------------------------------------
K_SWEEP = range(-12, 17)
# Measured on an MI355X (include/giga_hip.h, precision 2): the input scales 2^k at which the planes of the builder's weights
# (range ~3 at k = 0) meet the mode's tolerance.  fp16x3: 2.5e-5 at k = -8, 5.5e-5 at -9 (operands under 2^-3 keep 2^-25
# absolute), 7e-7 up to k = 14, NaN / inf from 15 (activations past 65520).  fp16: 7-9e-4 over the whole range up to 14.
WINDOW = {"fp16x3": (-8, 14), "fp16": (-12, 14)}
# plain f16 planes: range-relative bound inside the window (measured worst 8.8e-4, x 2, rounded up)
F16_PLANES_REL = 2e-3


def _window_check(k, lo, hi, tol, e, e_fin, where):
    """Below the window precision degrades gracefully (operands under 2^-3 keep 2^-25 absolute: at most 2x per halving of the
    scale); inside it the tolerance holds; above it every finite entry still meets the tolerance -- an overflow must show
    as NaN / inf, never as a finite wrong number."""
    if k < lo:
        return [("below", k, where, e)] if e > tol * 2.0 ** (lo - k + 1) else []
    if k <= hi:
        return [("inside", k, where, e)] if e > tol else []
    return [("finite-wrong", k, where, e_fin)] if e_fin > tol else []


def _window_tol(prec):
    return ref64.TOL["fp16x3"] if prec == "fp16x3" else F16_PLANES_REL


@pytest.mark.parametrize("prec", ["fp16x3", "fp16"])
def test_f16_encoder_scale_window(dev, prec):
    """x 2^k, k = -12..16, zero biases, by _window_check.  (Before the f16-class ReLUs and pools propagated NaN, plain fp16 at
    k = 15, 16 returned finite planes 0.5 of their range off next to NaN ones.)"""
    net = _configure(_net("nobias", dev), prec, "auto", False)
    x = torch.from_numpy(np.concatenate([ref64.input_family("uniform", 2), ref64.input_family("structured", 2, 5)]))
    ref = ref64.encoder(ref64.weight_family("nobias"), x)
    tol = _window_tol(prec)
    lo, hi = WINDOW[prec]
    bad = []
    try:
        for k in K_SWEEP:
            s = 2.0 ** k
            with torch.no_grad():
                pl = net.encode_inputs(x.to(dev) * s)
            torch.cuda.synchronize()
            for b in range(x.shape[0]):
                got = torch.stack([pl[key][b].double().cpu() for key in O.PLANES])
                want = torch.stack([ref[key][b] for key in O.PLANES]) * s
                e = ref64.range_err(got, want)
                e_fin, _ = ref64.finite_err(got, want)
                _record((prec, "window", "encoder", k), e)
                bad += _window_check(k, lo, hi, tol, e, e_fin, b)
    finally:
        _configure(net, "fp32", "auto", False)
    assert not bad, bad


# Decoder window on planes of range ~6 (standard normal) x 2^k, measured: fp16x3 3.1e-5 at k = -10, 7.2e-5 at -11, 2.3e-6
# up to 12, NaN / inf from 13; fp16 5-6e-4 over -12..12, NaN / inf from 13.
DEC_WINDOW = {"fp16x3": (-10, 12), "fp16": (-12, 12)}


@pytest.mark.parametrize("prec", ["fp16x3", "fp16"])
def test_f16_decoder_scale_window(dev, prec):
    """The decoders on foreign planes (giga_planes_pack) scaled by 2^k, zero biases and fc_p: raw logits against float64, the
    same rule as the encoder window.  (Before the f16-class decoder ReLUs propagated NaN, k = 15, 16 returned finite zeros in
    both modes: the integer ReLU turned the NaN of an overflowed layer into 0.)"""
    net = _configure(_net("nobias-nofcp", dev), prec, "auto", False)
    sd = ref64.weight_family("nobias-nofcp")
    g = torch.Generator().manual_seed(43)
    planes = {k: torch.randn(3, 32, 40, 40, generator=g) for k in O.PLANES}
    p = torch.from_numpy(synth.query_points(5, 3, 2048, stream=1, half_width=0.6))
    raw, _ = ref64.heads(sd, planes, p)
    tol = ref64.TOL["fp16x3"] if prec == "fp16x3" else F16_REL
    lo, hi = DEC_WINDOW[prec]
    bad = []
    try:
        for k in K_SWEEP:
            s = 2.0 ** k
            with torch.no_grad():
                got = {h: getattr(net, h)(p.to(dev), {key: (v * s).to(dev) for key, v in planes.items()}) for h in ref64.HEADS}
            torch.cuda.synchronize()
            for h in ref64.HEADS:
                for b in range(3):
                    gt = got[h][b].double().cpu()
                    e = ref64.range_err(gt, raw[h][b] * s)
                    e_fin, _ = ref64.finite_err(gt, raw[h][b] * s)
                    _record((prec, "window", "decoder", h, k), e)
                    bad += _window_check(k, lo, hi, tol, e, e_fin, (h, b))
    finally:
        _configure(net, "fp32", "auto", False)
    assert not bad, bad
