"""The lattice entry of the decoder (giga_decoder_forward_lattice: lattice_resample*_kernel, then launch_decoder with R > 0) at
every grid size it accepts, against float64 (tests/ref64.py) and against the generic gather of the same points.

Every case asserts two things.  (1) The outputs meet the project's tolerance against float64 heads on the explicitly expanded
points meshgrid(lin, lin, lin, 'ij'): ref64.TOL for 'fp32' / 'fp16x3', F16_REL of tests/test_gpu_envelope.py for the plain-f16
decoders, range-relative per scene and output (ref64.range_err; quaternions by ref64.rot_err, as the envelope test compares
them on a lattice).  (2) The same points as a plain (B, R^3, 3) tensor, one coordinate nudged so that the lattice detection
declines, give the same outputs through the generic kernels of the same precision, to the bounds of
tests/test_gpu_parity.py::test_lattice_fast_path_equals_generic_path (absolute: 2e-5, 2e-5, 1.5e-2); the nudged point is left
out.  An indexing slip fails (2) whatever the arithmetic does.  LATTICE_STATS proves which path each call took.

Lattices of one or two points per axis have outputs of (nearly) no range of their own: their errors are divided by the range of
the same scene's float64 outputs on the 8^3 planner lattice instead (`_companion`).

`plan` asks the library what a launch will do (convonet.decoder_plan: csrc/giga_dec_plan.h, the policy launch_decoder itself runs);
tests/test_lattice_host.py::test_dispatch_cases_cover_every_branch proves from it, on the CPU, that the cases below take every
lat_parts value, every `slots` branch and both settings of the XCD remap of decoder_lat_kernel.

Deviations from a plain product of cases, and why:
  * family c (unsorted, duplicated) needs five entries, so R = 1 and 2 run families a and b only;
  * 'adversarial' inputs are used from three scenes up (one scene of it is the empty volume alone);
  * 'fp16x3+fp16' has no generic path of its own precision; its assertion (2) is range-relative (see MIXED below);
  * the bit-for-bit batch check needs the same kernel on both sides.  Plain 'fp16' on decoder_lat_kernel therefore forces
    GIGA_DEC_LAT=1 for both calls (by default one scene alone, B < 4, runs decoder_f16s_kernel, another summation order); the
    shared-feature decoder_f16_kernel is checked at R = 64, where one scene alone (8192 tiles x 4 heads) is already past its
    16000-tile threshold.

No case needed its weight family restricted, and no kernel or launcher defect showed.  Measured on an MI355X (the LATTICE lines
this module prints; worst over the cases, smallest .. largest over R):
  kernel (LATTICE = true)        precision     against float64            lattice path against generic path
  decoder_f32_kernel             fp32          5.4e-7 .. 3.1e-6 (R = 64)  0 (bit for bit) from R = 2; 6.7e-7 at R = 1, where the
                                                                          generic call is one query per scene: the point kernel
  decoder_f16s_kernel            fp16x3        2.0e-7 .. 3.3e-6 (R = 64)  0 at every R
  decoder_f16s_kernel            fp16          3.3e-4 .. 1.7e-3 (R = 33)  0 at every R
  decoder_f16_kernel (shared)    fp16          1.5e-3 .. 2.0e-3 (R = 64)  0 at R = 41, 48, 63, 64
  decoder_lat_kernel             fp16x3        1.9e-6 .. 2.7e-6 (R = 40)  1.8e-6 .. 7.0e-6 (R = 32)
  decoder_lat_kernel             fp16          1.7e-3 .. 1.8e-3 (R = 32)  8.7e-4 .. 5.3e-3 (R = 40)
  decoder_lat_kernel             fp16x3+fp16   8.1e-4 .. 1.6e-3 (R = 32)  MIXED_GENERIC_FIGURE
  decoder_lat_kernel against decoder_f16s_kernel<LATTICE> (GIGA_DEC_LAT=0), fp16x3: 1.4e-6, 2.7e-6, 5.2e-6 at R = 8, 24, 40
  generic kernel at 65 samples per axis (value_grid), fp32: 1.3e-6 against float64
Bounds: 3.5e-5 (fp32, fp16x3) and 1e-2 (plain-f16 decoders) against float64; 2e-5 / 2e-5 / 1.5e-2 against the generic path."""
import ctypes
import os
import sys

import pytest
import torch

from giga_amd import _capi, convonet, networks
from giga_amd.detection import predict_batch
from giga_amd.generation import Generator3D

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402
from lattice_lins import grid_points, lin_family  # noqa: E402
from test_gpu_envelope import F16_REL  # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("qual", "rot", "width", "tsdf")
HEAD_OF = dict(zip(OUTS, ref64.HEADS))
PREC_CODE = {"fp32": 0, "fp16": 1, "fp16x3": 2, "fp16x3+fp16": 1}        # `precision` of the lattice decoder (giga_hip.h)
# tests/test_gpu_parity.py::test_lattice_fast_path_equals_generic_path
FAST_VS_GENERIC = {"fp32": 2e-5, "fp16x3": 2e-5, "fp16": 1.5e-2}
# 'fp16x3+fp16' has no generic path of its own precision: its lattice decoder is the plain-f16 one, its generic decoder the f16x3
# one, fp32-grade (within ref64.TOL of float64).  The generic outputs therefore stand in for float64 there, and the lattice outputs
# are held to them by the rule plain-f16 arithmetic is held to float64 by: range-relative, F16_REL (quaternions weighted by the
# float64 raw norm, so on the scenes that have a float64 reference).
MIXED = "fp16x3+fp16"
# how a head set is reached -> (outputs, heads per decoder launch)
MASKS = {"15": (OUTS, (3, 1)),          # net(x, pos, p_tsdf=pos): the grasp launch (mask 7) and the occupancy launch (mask 8)
         "7": (OUTS[:3], (3,)),         # predict_batch
         "8": (OUTS[3:], (1,)),         # decode_occ on cached planes
         "15x": (OUTS, (4,))}           # convonet.decode_heads with all four heads in ONE launch


# ---- the launch plan, from the library ---------------------------------------------------------------------------------
SHORT = {"decoder_lat_kernel": "lat", "decoder_f16s_kernel": "f16s", "decoder_f16_kernel": "f16", "decoder_f32_kernel": "f32"}


def plan(code, B, R, nheads):
    """convonet.decoder_plan of a lattice launch of precision `code` (csrc/giga_dec_plan.h, through giga_decoder_plan: host only;
    GIGA_DEC_LAT and the other knobs are read from the environment as the launch itself reads them), `kernel` shortened."""
    d = convonet.decoder_plan(B, 0, R, nheads, code)
    d["kernel"] = SHORT[d["kernel"]]
    return d


# ---- cases --------------------------------------------------------------------------------------------------------------
# decoder_lat_kernel: 'fp16x3' at any B, plain 'fp16' (and 'fp16x3+fp16') from 4 scenes up; R in {8, 16, 24, 32, 40}.
# The policy per launch (nh = heads of the launch; cap = 256 / nh, cap8 = 256 / (8 nh) * 8; ntile = (R/4)(R/8); lat_parts = the c of
# {1, 2, 5} dividing ntile with the least ceil(B R c / cap) * (ntile / c + 12); nslab = B R lat_parts; slots = nslab if nslab < cap,
# else cap8 if nslab >= 2 cap8, else cap; XCD remap iff slots * nh % (8 nh) == 0), written out by hand for every launch of
# LAT_CASES: tests/test_lattice_host.py::test_lat_table_equals_the_plan holds the plan to these rows, so a change of the policy
# shows here.
# (R, B, mask, nh, ntile, lat_parts, nslab, slots, branch of `slots`, XCD remap)
LAT_TABLE = [
    (8, 1, "15", 3, 2, 2, 16, 16, "nslab", True),
    (8, 1, "15", 1, 2, 2, 16, 16, "nslab", True),
    (8, 13, "15", 3, 2, 1, 104, 85, "cap", False),
    (8, 13, "15", 1, 2, 2, 208, 208, "nslab", True),
    (8, 5, "15x", 4, 2, 1, 40, 40, "nslab", True),
    (16, 1, "7", 3, 8, 2, 32, 32, "nslab", True),
    (16, 4, "15", 3, 8, 1, 64, 64, "nslab", True),
    (16, 4, "15", 1, 8, 2, 128, 128, "nslab", True),
    (16, 13, "7", 3, 8, 1, 208, 80, "cap8", True),
    (24, 1, "8", 1, 18, 2, 48, 48, "nslab", True),
    (24, 5, "15", 3, 18, 1, 120, 85, "cap", False),
    (24, 5, "15", 1, 18, 2, 240, 240, "nslab", True),
    (24, 13, "8", 1, 18, 1, 312, 256, "cap", True),
    (32, 1, "15x", 4, 32, 2, 64, 64, "cap", True),
    (32, 4, "15", 3, 32, 1, 128, 85, "cap", False),
    (32, 4, "15", 1, 32, 2, 256, 256, "cap", True),
    (32, 5, "7", 3, 32, 1, 160, 80, "cap8", True),
    (40, 1, "15", 3, 50, 2, 80, 80, "nslab", True),
    (40, 1, "15", 1, 50, 5, 200, 200, "nslab", True),
    (40, 5, "15", 3, 50, 2, 400, 80, "cap8", True),
    (40, 5, "15", 1, 50, 1, 200, 200, "nslab", True),
    (40, 13, "15", 3, 50, 1, 520, 80, "cap8", True),
    (40, 13, "15", 1, 50, 2, 1040, 256, "cap8", True),
]
# (R, B, mask, lin family, weight family, input family, precisions)
LAT_CASES = [
    (8, 1, "15", "a", "he-7", "realistic", ("fp16x3",)),
    (8, 13, "15", "c", "nobias", "adversarial", ("fp16x3", "fp16")),
    (8, 5, "15x", "b", "he-7", "adversarial", ("fp16x3", "fp16")),
    (16, 1, "7", "a", "nobias", "realistic", ("fp16x3",)),
    (16, 4, "15", "c", "he-7", "adversarial", ("fp16x3", "fp16")),
    (16, 13, "7", "b", "he-7", "realistic", ("fp16", MIXED)),
    (24, 1, "8", "a", "he-7", "realistic", ("fp16x3",)),
    (24, 5, "15", "c", "he-7", "realistic", ("fp16x3", "fp16")),
    (24, 13, "8", "b", "nobias", "realistic", ("fp16x3", "fp16")),
    (32, 1, "15x", "b", "he-7", "realistic", ("fp16x3",)),
    (32, 4, "15", "a", "he-7", "realistic", ("fp16x3", "fp16", MIXED)),
    (32, 5, "7", "c", "nobias", "adversarial", ("fp16x3", "fp16")),
    (40, 1, "15", "a", "he-7", "realistic", ("fp16x3",)),
    (40, 5, "15", "c", "nobias", "adversarial", ("fp16x3", "fp16")),
    (40, 13, "15", "b", "he-7", "realistic", ("fp16", MIXED)),
]
# The LATTICE = true instantiations of decoder_f32_kernel / decoder_f16s_kernel / decoder_f16_kernel: fp32 at every R, the
# f16-class modes where R % 8 != 0 or R > 40, plain fp16 below 4 scenes.  (48, 2, "15") in plain fp16 is the shared-feature kernel
# (decoder_f16_kernel: tiles * heads = 6912 * 3 >= 16000) for the grasp heads and the head-resident one for the occupancy head.
ALL3 = ("fp32", "fp16x3", "fp16")
GEN_CASES = [
    (1, 1, "15", "a", "he-7", "realistic", ALL3),
    (1, 3, "8", "b", "nobias", "adversarial", ("fp32", "fp16")),
    (2, 3, "7", "a", "he-7", "adversarial", ALL3),
    (2, 1, "15", "b", "nobias", "realistic", ("fp16x3", "fp16")),
    (7, 3, "15", "c", "he-7", "realistic", ALL3),
    (7, 1, "8", "a", "nobias", "realistic", ("fp32", "fp16x3")),
    (9, 3, "15", "b", "nobias", "adversarial", ALL3),
    (9, 1, "7", "c", "he-7", "realistic", ("fp32", "fp16")),
    (17, 3, "15", "c", "he-7", "adversarial", ALL3),
    (17, 1, "15", "a", "nobias", "realistic", ALL3),
    (17, 3, "8", "b", "he-7", "realistic", ("fp16x3", "fp16")),
    (33, 1, "15", "c", "he-7", "realistic", ALL3),
    (33, 3, "7", "a", "nobias", "adversarial", ALL3),
    (41, 3, "15", "b", "he-7", "realistic", ALL3),
    (41, 1, "8", "c", "nobias", "realistic", ("fp32", "fp16x3")),
    (48, 1, "15", "a", "he-7", "realistic", ALL3),
    (48, 2, "15", "c", "he-7", "realistic", ALL3),
    (48, 3, "7", "b", "nobias", "adversarial", ("fp32", "fp16")),
    (63, 3, "15", "c", "he-7", "realistic", ALL3),
    (63, 1, "7", "b", "nobias", "realistic", ("fp16x3", "fp16")),
    (64, 3, "15", "a", "he-7", "adversarial", ALL3),
    (64, 1, "8", "c", "he-7", "realistic", ALL3),
]


def _expand(cases):
    return [pytest.param(c[:6], prec, id="R{}-B{}-m{}-{}-{}-{}-{}".format(*c[:6], prec)) for c in cases for prec in c[6]]


# ---- fixtures and caches ------------------------------------------------------------------------------------------------
_MEASURED = {}


def _record(key, err):
    _MEASURED[key] = max(_MEASURED.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nLATTICE worst errors per kernel / precision / R (f64: range-relative against float64; generic: absolute against the "
          "generic path):")
    for k, v in sorted(_MEASURED.items(), key=lambda kv: (kv[0][0], kv[0][1], kv[0][2], kv[0][3])):
        print("LATTICE", "/".join(map(str, k)), f"{v:.3e}")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


_NETS, _PLANES, _REF, _POS = {}, {}, {}, {}


def _net(wfam, dev):
    if wfam not in _NETS:
        n = networks.get_network("giga")
        n.load_state_dict(ref64.weight_family(wfam))
        _NETS[wfam] = n.to(dev).eval()
    return _NETS[wfam]


def _pos(R, fam, dev):
    """The registered (1, R^3, 3) device lattice of a family, and its fp32 `lin` on the host."""
    if (R, fam) not in _POS:
        lin = lin_family(fam, R)
        _POS[(R, fam)] = (convonet.register_lattice(grid_points(lin).to(dev), lin), lin)
    return _POS[(R, fam)]


def _scenes(B):
    return list(range(B)) if B <= 5 else [0, B // 2, B - 1]


def _planes64(wfam, ifam, B):
    """(x, float64 planes of the sampled scenes), cached per module."""
    key = (wfam, ifam, B)
    if key not in _PLANES:
        x = torch.from_numpy(ref64.input_family(ifam, B))
        _PLANES[key] = (x, ref64.encoder(ref64.weight_family(wfam), x[_scenes(B)]))
    return _PLANES[key]


def _reference(wfam, ifam, B, R, fam, outs):
    """float64 (raw, out) of the heads behind `outs` on meshgrid(lin, lin, lin, 'ij') of the sampled scenes, cached per module
    and left unchanged; the points are expanded from the same fp32 lin values the device gets."""
    key = (wfam, ifam, B, R, fam, outs)
    if key not in _REF:
        _, planes = _planes64(wfam, ifam, B)
        p = grid_points(lin_family(fam, R)).expand(len(_scenes(B)), -1, -1)
        _REF[key] = ref64.heads(ref64.weight_family(wfam), planes, p, tuple(HEAD_OF[o] for o in outs))
    return _REF[key]


def _companion(wfam, ifam, B, outs):
    """The same scenes' float64 outputs on the 8^3 planner lattice: the range that errors of one- and two-point-per-axis
    lattices are divided by."""
    return _reference(wfam, ifam, B, 8, "a", outs)[1]


def _run(net, prec, mask, x, pts):
    """{output: (B, N[, 4]) device tensor} of the head set `mask` at `pts` (a registered lattice or a plain (B, N, 3) tensor)."""
    with torch.no_grad():
        if mask == "15":
            return dict(zip(OUTS, net(x, pts, p_tsdf=pts)))
        if mask == "7":
            return dict(zip(OUTS, predict_batch(x, pts, net)))
        c = net.encode_inputs(x)
        if mask == "8":
            return {"tsdf": net.decode_occ(pts, c).logits}
        got = convonet.decode_heads(c.nhwc, pts, net.packed_blob(x.device), 15, prec, post=True)
        return {o: got[HEAD_OF[o]] for o in OUTS}


def _rel_err(what, got, want, rng_of, raw=None):
    """max |got - want| / range(rng_of) of one scene's output (inf when got has a non-finite entry); quaternions with each point's
    error weighted by |raw| / max |raw| over the scene, raw = the float64 raw quaternions of the points compared.  With
    rng_of = want (and raw the reference's) this is ref64.range_err / ref64.rot_err; the other callers compare a part of a scene,
    or two device outputs, over the range of the scene's float64 reference."""
    g, r = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    d = (g - r).abs()
    if what == "rot":
        d = d * raw[0] / raw[1]
    return d.max().item() / max((rng_of.max() - rng_of.min()).item(), 1e-30)


def _rot_weights(ref_raw, j):
    """(|raw| per point (N, 1), its maximum) of scene slot j's float64 raw quaternions."""
    n = ref_raw["decoder_rot"][j].norm(dim=-1, keepdim=True)
    return n, n.max()


def _tol(prec):
    return ref64.TOL[prec] if prec in ref64.TOL else F16_REL


def _plain_points(pos, B, R):
    """The lattice as a plain (B, R^3, 3) tensor that takes the generic path, and the index of the point to leave out of the
    comparison (None below R = 8, where the detection declines by itself and nothing is nudged)."""
    plain = pos.expand(B, -1, -1).clone()
    if R < 8:
        return plain, None
    j = R ** 3 // 2 + 3
    plain[0, j, 1] += 1e-3
    return plain, j


def _check_case(dev, case, prec):
    """Both assertions of the module docstring for one case; returns the lattice-path outputs."""
    R, B, mask, fam, wfam, ifam = case
    outs, launches = MASKS[mask]
    net = _net(wfam, dev)
    pos, _ = _pos(R, fam, dev)
    x, _ = _planes64(wfam, ifam, B)
    ks = _scenes(B)
    ref_raw, ref_out = _reference(wfam, ifam, B, R, fam, outs)
    rng_out = _companion(wfam, ifam, B, outs) if R <= 2 else None
    plain, skip = _plain_points(pos, B, R)
    xd = x.to(dev)
    net.set_precision(prec)
    try:
        s0 = dict(convonet.LATTICE_STATS)
        fast = _run(net, prec, mask, xd, pos)
        s1 = dict(convonet.LATTICE_STATS)
        slow = _run(net, prec, mask, xd, plain)
        s2 = dict(convonet.LATTICE_STATS)
        torch.cuda.synchronize()
    finally:
        net.set_precision("fp32")
    assert (s1["fast"] - s0["fast"], s1["generic"] - s0["generic"]) == (len(launches), 0), (s0, s1)
    assert (s2["fast"] - s1["fast"], s2["generic"] - s1["generic"]) == (0, len(launches)), (s1, s2)
    N = R ** 3
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    if skip is not None:
        keep[skip] = False
    fails = []
    for what in outs:
        nh = launches[0] if what != "tsdf" or len(launches) == 1 else launches[1]
        form = plan(PREC_CODE[prec], B, R, nh)["kernel"]
        a, b = fast[what], slow[what]
        assert a.shape == b.shape and a.shape[:2] == (B, N), (what, a.shape, b.shape)
        h = HEAD_OF[what]
        # (2) lattice path against generic path
        if prec == MIXED:
            for k in (ks if what == "rot" else range(B)):
                if what == "rot":
                    n, nmax = _rot_weights(ref_raw, ks.index(k))
                    d = _rel_err(what, a[k, keep], b[k, keep], ref_out[h][ks.index(k)], (n[keep.cpu()], nmax))
                else:
                    d = _rel_err(what, a[k, keep], b[k, keep], b[k, keep].double().cpu())
                _record((form, prec, R, "generic (range-relative)"), d)
                if not d <= F16_REL:
                    fails.append(("generic", what, k, d))
        else:
            d = (a[:, keep] - b[:, keep]).abs().max().item() if bool(torch.isfinite(a).all()) else float("inf")
            _record((form, prec, R, "generic"), d)
            if not d <= FAST_VS_GENERIC[prec]:
                fails.append(("generic", what, d))
        # (1) float64
        for j, k in enumerate(ks):
            raw = _rot_weights(ref_raw, j) if what == "rot" else None
            if rng_out is None:
                e = ref64.rot_err(a[k], ref_out[h][j], ref_raw[h][j]) if what == "rot" else ref64.range_err(a[k], ref_out[h][j])
            else:
                e = _rel_err(what, a[k], ref_out[h][j], rng_out[h][j], raw)
            _record((form, prec, R, "f64"), e)
            if not e <= _tol(prec):
                fails.append(("f64", what, k, e))
            if R % 2 == 1:
                # The last 32 outputs of every scene, where the ragged tail tile of an odd lattice lives, spelled out: the same
                # error over those points alone, still divided by the whole scene's range.  The assertion above implies it; it
                # is kept so that a failure names the tail.
                rng = (rng_out if rng_out is not None else ref_out)[h][j]
                t = _rel_err(what, a[k, -32:], ref_out[h][j][-32:], rng, (raw[0][-32:], raw[1]) if raw else None)
                if not t <= _tol(prec):
                    fails.append(("tail", what, k, t))
                if prec != MIXED:                              # (the mixed mode runs decoder_lat_kernel only: no odd size)
                    tg = (a[k, -32:] - b[k, -32:]).abs().max().item()
                    if not tg <= FAST_VS_GENERIC[prec]:
                        fails.append(("tail-generic", what, k, tg))
    assert not fails, fails
    return fast


# ---- the sweeps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,prec", _expand(LAT_CASES))
def test_lat_kernel_matches_float64_and_generic(dev, case, prec):
    """decoder_lat_kernel at R = 8 .. 40: every lat_parts value, `slots` branch and XCD setting of the table above."""
    _check_case(dev, case, prec)


@pytest.mark.parametrize("case,prec", _expand(GEN_CASES))
def test_lattice_forms_match_float64_and_generic(dev, case, prec):
    """The LATTICE = true kernels at R = 1 .. 64: odd sizes (ragged last tile, magic division), sizes below the detection
    limit (registered lattices only) and above decoder_lat_kernel's."""
    _check_case(dev, case, prec)


@pytest.mark.parametrize("case", [LAT_CASES[1][:6], LAT_CASES[7][:6], LAT_CASES[13][:6]], ids=["R8", "R24", "R40"])
def test_lat_kernel_equals_head_resident_lattice_kernel(dev, case, monkeypatch):
    """GIGA_DEC_LAT is read per call: the same fp16x3 inputs on decoder_lat_kernel and, with GIGA_DEC_LAT=0, on
    decoder_f16s_kernel<LATTICE> agree to the fast-versus-generic bound, and each meets the float64 tolerance."""
    R, B, mask = case[:3]
    assert R in (8, 24, 40) and case[3] == "c"
    monkeypatch.delenv("GIGA_DEC_LAT", raising=False)
    assert all(plan(2, B, R, nh)["kernel"] == "lat" for nh in MASKS[mask][1])
    lat = _check_case(dev, case, "fp16x3")
    monkeypatch.setenv("GIGA_DEC_LAT", "0")
    assert all(plan(2, B, R, nh)["kernel"] == "f16s" for nh in MASKS[mask][1])
    res = _check_case(dev, case, "fp16x3")
    for what in MASKS[mask][0]:
        d = (lat[what] - res[what]).abs().max().item()
        _record(("lat-vs-f16s", "fp16x3", R, "generic"), d)
        assert d <= FAST_VS_GENERIC["fp16x3"], (what, d)


# ---- batch behaviour ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,prec,R,B,force", [("lat", "fp16x3", 24, 5, None), ("lat", "fp16", 16, 4, "1"),
                                                 ("f16s", "fp16x3", 17, 3, None), ("f16s", "fp16", 17, 3, None),
                                                 ("f16", "fp16", 64, 2, None), ("f32", "fp32", 17, 3, None)],
                         ids=["lat-fp16x3", "lat-fp16", "f16s-fp16x3", "f16s-fp16", "f16-shared-fp16", "f32"])
def test_scene_of_a_batch_equals_the_scene_alone(dev, monkeypatch, form, prec, R, B, force):
    """All four heads on the cached planes of ONE batched encode_inputs: scene k of the batch equals the same decode_heads call on
    scene k's planes alone -- bit for bit in the f16-class modes (the same kernel on both sides: see the module docstring for
    plain fp16), to 2e-5 in fp32."""
    if force is None:
        monkeypatch.delenv("GIGA_DEC_LAT", raising=False)
    else:
        monkeypatch.setenv("GIGA_DEC_LAT", force)
    assert plan(PREC_CODE[prec], B, R, 4)["kernel"] == form and plan(PREC_CODE[prec], 1, R, 4)["kernel"] == form
    net = _net("he-7", dev)
    pos, _ = _pos(R, "c", dev)
    x = torch.from_numpy(ref64.input_family("realistic", B)).to(dev)
    net.set_precision(prec)
    try:
        with torch.no_grad():
            c = net.encode_inputs(x)
            blob = net.packed_blob(dev)
            before = convonet.LATTICE_STATS["fast"]
            whole = convonet.decode_heads(c.nhwc, pos, blob, 15, prec, post=True)
            alone = [convonet.decode_heads(c.nhwc[:, k:k + 1].contiguous(), pos, blob, 15, prec, post=True) for k in range(B)]
            assert convonet.LATTICE_STATS["fast"] - before == B + 1
        torch.cuda.synchronize()
    finally:
        net.set_precision("fp32")
    for h in ref64.HEADS:
        for k in range(B):
            a, b = whole[h][k], alone[k][h][0]
            assert bool(torch.isfinite(a).all())
            if prec == "fp32":
                assert (a - b).abs().max().item() <= 2e-5, (h, k)
            else:
                assert torch.equal(a, b), (h, k, (a - b).abs().max().item())


# ---- the entry point through ctypes ---------------------------------------------------------------------------------------
SENTINEL = 0x7FA5C3D2          # a NaN payload no kernel produces
PAD = 1024                     # words (outputs) / bytes x 4 (workspace) of sentinel on either side


def _embedded_f32(n, dev):
    """(buffer of int32 sentinels, pointer to the n floats in its middle)."""
    buf = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.int32, device=dev)
    return buf, ctypes.c_void_p(buf.data_ptr() + 4 * PAD)


def _untouched(buf, lo, hi):
    """Every word of `buf` outside [lo, hi) still holds the sentinel."""
    return bool((buf[:lo] == SENTINEL).all()) and bool((buf[hi:] == SENTINEL).all())


def _lattice_call_buffers(dev, B, R, prec_flags, seed):
    code = prec_flags & 3
    L = _capi.lib()
    g = torch.Generator().manual_seed(seed)
    planes = torch.randn(3, B, 40, 40, 32, generator=g).to(dev)
    if code == 1 and not prec_flags & _capi.PLANES_FP32:
        planes = planes.half()
    N = R ** 3
    outs = [_embedded_f32(B * N * w, dev) for w in (1, 4, 1, 1)]
    wsb = L.giga_lattice_workspace_bytes(B, R, prec_flags)
    assert wsb == 3 * B * R * R * 32 * (2 if code == 1 else 4)
    ws = torch.full((PAD + wsb // 4 + PAD,), SENTINEL, dtype=torch.int32, device=dev)
    return planes, outs, ws, wsb


@pytest.mark.parametrize("label,prec_flags,R,B,force", [("fp32", 0, 9, 3, None), ("fp16", 1, 9, 3, None), ("fp16x3", 2, 9, 3, None),
                                                        ("fp16+planes32", 1 | _capi.PLANES_FP32, 9, 3, None),
                                                        ("lat-fp16x3", 2, 40, 1, None), ("lat-fp16", 1, 40, 1, "1")],
                         ids=["fp32", "fp16", "fp16x3", "fp16+planes32", "lat-fp16x3", "lat-fp16"])
def test_writes_stay_inside_outputs_and_workspace(dev, monkeypatch, label, prec_flags, R, B, force):
    """giga_decoder_forward_lattice with valid arguments, every output and the exactly sized workspace embedded in larger
    sentinel-filled device buffers: nothing outside the exact extents changes, and every output element is written."""
    if force is None:
        monkeypatch.delenv("GIGA_DEC_LAT", raising=False)
    else:
        monkeypatch.setenv("GIGA_DEC_LAT", force)
    assert (plan(prec_flags & 3, B, R, 4)["kernel"] == "lat") == label.startswith("lat")
    L = _capi.lib()
    net = _net("he-7", dev)
    blob = net.packed_blob(dev)
    lin = lin_family("c", R).to(dev)
    planes, outs, ws, wsb = _lattice_call_buffers(dev, B, R, prec_flags, seed=R + B)
    torch.cuda.synchronize()
    with torch.cuda.device(dev):
        rc = L.giga_decoder_forward_lattice(_capi.ptr(planes), _capi.ptr(lin), _capi.ptr(blob), 15,
                                            outs[0][1], outs[1][1], outs[2][1], outs[3][1], B, R, prec_flags, 1,
                                            ctypes.c_void_p(ws.data_ptr() + 4 * PAD), wsb, _capi.stream_ptr(dev), None, None)
    torch.cuda.synchronize()
    assert rc == 0
    for (buf, _), w in zip(outs, (1, 4, 1, 1)):
        n = B * R ** 3 * w
        assert _untouched(buf, PAD, PAD + n), w
        body = buf[PAD:PAD + n]
        assert not bool((body == SENTINEL).any()), w
        assert bool(torch.isfinite(body.view(torch.float32)).all()), w
    assert _untouched(ws, PAD, PAD + wsb // 4)
    assert not bool((ws[PAD:PAD + wsb // 4] == SENTINEL).any())       # the resampled planes fill the workspace


def test_entry_point_argument_handling(dev):
    """Calls that return before anything is enqueued: the code, and sentinel-filled outputs and workspace left untouched."""
    L = _capi.lib()
    for code in (0, 1, 2):
        for R in (1, 9, 64):
            for B in (1, 3):
                assert L.giga_lattice_workspace_bytes(B, R, code) == 3 * B * R * R * 32 * (2 if code == 1 else 4)
    assert L.giga_lattice_workspace_bytes(0, 9, 0) == 0 and L.giga_lattice_workspace_bytes(3, 0, 2) == 0
    B, R = 3, 9
    blob = _net("he-7", dev).packed_blob(dev)
    lin = lin_family("a", R).to(dev)
    planes, outs, ws, wsb = _lattice_call_buffers(dev, B, R, 0, seed=1)
    wsp = ctypes.c_void_p(ws.data_ptr() + 4 * PAD)

    def call(R_=R, wsb_=wsb, qual=outs[0][1], mask=15):
        with torch.cuda.device(dev):
            rc = L.giga_decoder_forward_lattice(_capi.ptr(planes), _capi.ptr(lin), _capi.ptr(blob), mask, qual, outs[1][1],
                                                outs[2][1], outs[3][1], B, R_, 0, 1, wsp, wsb_, _capi.stream_ptr(dev), None, None)
        torch.cuda.synchronize()
        return rc

    assert call(R_=65) == -1
    assert call(R_=0) == 0
    assert call(wsb_=wsb - 1) == -4
    assert call(qual=None) == -6
    for buf, _ in outs:
        assert bool((buf == SENTINEL).all())
    assert bool((ws == SENTINEL).all())
    # the control: the very same buffers are valid arguments -- without the head whose pointer is null the call runs
    assert call(qual=None, mask=14) == 0
    assert bool((outs[0][0] == SENTINEL).all())
    for (buf, _), w in zip(outs[1:], (4, 1, 1)):
        assert _untouched(buf, PAD, PAD + B * R ** 3 * w) and not bool((buf[PAD:PAD + B * R ** 3 * w] == SENTINEL).any())


# ---- Generator3D around the 64-point limit --------------------------------------------------------------------------------
def test_occupancy_grid_small_and_too_large(dev):
    """grid_points registers any resolution: R = 4 (below the detection limit, reachable only through registration) runs the
    lattice decoder and matches float64 in every precision; occupancy_grid refuses more than 64 points per axis."""
    net = _net("he-7", dev)
    x, planes = _planes64("he-7", "realistic", 3)
    R = 4
    lin = torch.linspace(-0.5, 0.5, R)
    _, ref = ref64.heads(ref64.weight_family("he-7"), planes, grid_points(lin).expand(3, -1, -1), ("decoder_tsdf",))
    gen = Generator3D(net, device=dev)
    try:
        for prec in ("fp32", "fp16x3", "fp16"):
            net.set_precision(prec)
            c = gen.encode(x)
            before = dict(convonet.LATTICE_STATS)
            got = gen.occupancy_grid(c, resolution=R)
            assert convonet.LATTICE_STATS["fast"] - before["fast"] == 1 and convonet.LATTICE_STATS["generic"] == before["generic"]
            assert tuple(got.shape) == (3, R, R, R)
            for k in range(3):
                e = ref64.range_err(got[k].reshape(-1), ref["decoder_tsdf"][k])
                _record((plan(PREC_CODE[prec], 3, R, 1)["kernel"], prec, R, "f64"), e)
                assert e <= _tol(prec), (prec, k, e)
        net.set_precision("fp32")
        c = gen.encode(x)
        before = dict(convonet.LATTICE_STATS)
        with pytest.raises(_capi.GigaHipError):
            gen.occupancy_grid(c, resolution=65)
        assert dict(convonet.LATTICE_STATS) == before
    finally:
        net.set_precision("fp32")


def test_value_grid_above_the_lattice_limit_takes_the_generic_path(dev):
    """65 samples per axis (resolution0 = 65, upsampling_steps = 0): not registered, decoded by the generic kernel in one launch
    over both scenes, and equal to float64 on scene 0."""
    net = _net("he-7", dev)
    net.set_precision("fp32")
    x, planes = _planes64("he-7", "realistic", 3)
    gen = Generator3D(net, device=dev, resolution0=65, upsampling_steps=0)
    c = gen.encode(x[:2])
    before = dict(convonet.LATTICE_STATS)
    grid = gen.value_grid(c)
    torch.cuda.synchronize()
    after = dict(convonet.LATTICE_STATS)
    assert (after["generic"] - before["generic"], after["fast"] - before["fast"], after["detected"] - before["detected"]) == (1, 0, 0)
    assert tuple(grid.shape) == (2, 65, 65, 65)
    lin = ((1 + 0.1) * torch.linspace(-0.5, 0.5, 65)).float()
    _, ref = ref64.heads(ref64.weight_family("he-7"), {k: v[:1] for k, v in planes.items()}, grid_points(lin), ("decoder_tsdf",))
    e = ref64.range_err(grid[0].reshape(-1), ref["decoder_tsdf"][0])
    _record(("generic-kernel", "fp32", 65, "f64"), e)
    assert e <= ref64.TOL["fp32"], e
