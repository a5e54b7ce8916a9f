"""The encoder backward held to float64 STAGE BY STAGE (tests/bwd_stage_ref.py), in the bf16 step (BASELINE c5) and the fp32
step: one training step per case, then each of the fifteen stages of the data-gradient chain

    L12 L11 L10 L9 L8 L7 L6 L5 L4 pool1 L3 L2 pool0 L1 L0

is checked on the buffers the GPU itself fed into it (forward activations: giga_encoder_workspace_layout; the plane gradients
at offset 0 of the backward workspace, then gA6 ... gP0: giga_backward_workspace_layout), so a bug in one stage fails that
stage and no other -- a dropped border tap, an unflipped tap, swapped halves of a concat gradient or a wrong mask changes one
stage by O(1) and can still pass the whole-network bounds (2 % relative L2, cosine > 0.9) the bf16 step is otherwise held to.
The plane gradients stay what the decoders left: no stage of encoder_backward_impl writes them (L12 and conv_final's weight
gradient only read them), which L12's own check and conv_final's bias gradient (their column sums) confirm on every case.
Also checked, with unrounded operands (they run the fp32 MFMA in both steps): the weight and bias gradients of the two
ConvTranspose layers and conv_final, which the layer-by-layer test of the 3x3 weight gradients does not walk.

Forms: one launch per stage in process (bf16: launch_conv<..., MATH_BF16>; fp32: Winograd F(2x2, 3x3) data gradients), and
GIGA_WINOGRAD_BWD=0 (fp32 direct kernels) in a child process, since the variable is read once per process.  A second child
sets every environment switch the library no longer reads to its former non-default value and must run the same forms as a
process without them.  giga_backward_last_path() must report the form every case expects.  Shapes (scenes -> images): 3 -> 9
(no multiple of 8: conv_wg_map's plain mapping; the training forward's per-layer launches), 8 -> 24 (XCD-local mapping; the
forward's persistent launch from here up: one image per group), 9 -> 27 (32 groups for 27 images: groups that return before any
barrier), 11 -> 33 (one group owns two images).  'he-7' weights, 'uniform' inputs at every size, 'structured' inputs
(pool ties, large zero regions of the masks) at 3 and 11 scenes; a smooth objective, 64 occupancy queries, one grasp query.

Tolerances (bwd_stage_ref.tol_bf16 / tol_fp32; tests/test_bwd_stage_host.py shows that each rejects every one-stage bug it
lists by >= 4x): bf16 convolution stages |got - want| <= 2e-5 max|want| + 1e-5 mag per element against the reference on
bf16-rounded operands; fp32 convolution stages 2e-5 max|want|; pool stages bit-equal; masked-out elements exactly zero."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from giga_amd import _capi, networks, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd_stage_ref as R  # noqa: E402
import ref64  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_GRASP, M_OCC = 1, 64
W, BF = _capi.BWD_PATH_WINOGRAD, _capi.BWD_PATH_BF16
# (scenes, input family) per form
PER_STAGE = [(3, "uniform"), (8, "uniform"), (9, "uniform"), (11, "uniform"), (3, "structured"), (11, "structured")]
DIRECT = [(3, "uniform"), (8, "uniform"), (3, "structured")]
# the switches of decided experiments, removed with the losing paths: (variable, its former non-default value)
RETIRED = {"GIGA_DGRAD_PERSIST": "1", "GIGA_BF16_CONVIN": "0", "GIGA_UNET_PERSIST": "0", "GIGA_CONV_XCD": "0", "GIGA_CONV32": "0",
           "GIGA_LAT_NW": "12"}


def run_step(prec, B, ifam):
    """One training step on cuda:0; returns (path bits, sd, acts, grads, parameter gradients) with the GPU's own buffers
    on the CPU: acts / grads {name: NCHW fp32} as bwd_stage_ref names them."""
    dev = torch.device("cuda:0")
    sd = ref64.weight_family("he-7")
    x = torch.from_numpy(ref64.input_family(ifam, B, first=500)).to(dev)
    pos = torch.from_numpy(synth.query_points(500, B, N_GRASP, stream=2)).to(dev)
    pos_occ = torch.from_numpy(synth.query_points(500, B, M_OCC, stream=3, half_width=0.55)).to(dev)
    net = networks.get_network("giga")
    net.load_state_dict(sd)
    net = net.to(dev).train().set_train_precision(prec)
    obj = ref64.smooth_objective(B, N_GRASP, M_OCC, seed=B)
    out = net(x, pos, p_tsdf=pos_occ)
    sum((o * obj[h].float().to(dev)).sum() for o, h in zip(out, ref64.HEADS)).backward()
    torch.cuda.synchronize()
    path = _capi.lib().giga_backward_last_path()
    sb = [b for b in net._train_state._pool if b.key == (B, N_GRASP, M_OCC)][-1]
    fo, bo = (ctypes.c_size_t * 17)(), (ctypes.c_size_t * 15)()
    assert _capi.lib().giga_encoder_workspace_layout(B, _capi.PRECISION[prec], fo) == 0
    assert _capi.lib().giga_backward_workspace_layout(B, bo) == 0

    def nchw(buf, off, c, h):
        n = 3 * B * h * h * c
        return buf[off:off + 4 * n].view(torch.float32).view(3 * B, h, h, c).permute(0, 3, 1, 2).cpu().contiguous()

    acts = {nm: nchw(sb.ws, fo[i], *R.ACT[nm]) for i, nm in enumerate(R.ACT_ORDER)}
    grads = {nm: nchw(sb.wsb, bo[i], *R.GRAD[nm]) for i, nm in enumerate(R.GRAD_ORDER)}
    grads["gOUT"] = nchw(sb.wsb, 0, *R.GRAD["gOUT"])           # the plane gradients come first
    pg = {n: q.grad.detach().cpu() for n, q in net.named_parameters() if n.startswith(R.PREFIX)}
    return path, sd, acts, grads, pg


def check_step(prec, B, ifam, expect_path, form):
    """Assert every stage of one step; returns {stage: worst error / tolerance}."""
    path, sd, acts, grads, pg = run_step(prec, B, ifam)
    tag = f"{form} {prec} B={B} {ifam}"
    assert path == expect_path, (tag, "giga_backward_last_path", path, expect_path)
    assert all(bool(torch.isfinite(t).all()) for t in grads.values()), tag
    assert float(grads["gOUT"].abs().max()) > 0 and float(grads["gP0"].abs().max()) > 0, tag
    r, tol_of = (R.bf16, R.tol_bf16) if prec == "bf16" else (None, R.tol_fp32)
    worst, bad = {}, []
    for st in R.STAGES:
        got = grads[st.dst]
        want, mag = R.stage_want(st, grads, acts, sd, r)
        if st.kind == "pool":
            assert want.dtype == torch.float32
            neq = got != want
            worst[st.name] = float("inf") if bool(neq.any()) else 0.0
            if bool(neq.any()):
                bad.append((st.name, "not bit-equal", int(neq.sum()), float((got - want).abs().max())))
            continue
        ratio = (got.double() - want).abs() / tol_of(want, mag)
        worst[st.name] = float(ratio.max())
        if not worst[st.name] <= 1.0:
            i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
            bad.append((st.name, worst[st.name], i, float(got[i]), float(want[i]), float(want.abs().max())))
        if st.mask and bool((got[~(acts[st.mask] > 0)] != 0).any()):
            bad.append((st.name, "masked-out elements not zero", int((got[~(acts[st.mask] > 0)] != 0).sum())))
    # the weight / bias gradients of the ConvTranspose layers and conv_final: fp32 MFMA on unrounded operands in both steps
    for e in R.WGRADS:
        for kind, (want, mag) in zip(("weight", "bias"), R.wgrad_want(e, grads, acts)):
            got = pg[R.PREFIX + e[2] + "." + kind].double()
            assert got.shape == want.shape, (e[0], kind)
            key = f"d{kind[0]}{e[0][1:]}"
            worst[key] = float(((got - want).abs() / R.tol_bf16(want, mag)).max())
            if not worst[key] <= 1.0:
                bad.append((key, worst[key], float(want.abs().max())))
    print(f"STAGES {tag} path {path}: " + " ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert not bad, (tag, bad)
    return worst


_WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nBACKWARD STAGES worst error / tolerance per form and stage:")
    for k, v in sorted(_WORST.items()):
        print("BWDSTAGE", k, f"{v:.3f}")


def _note(form, prec, worst):
    for k, v in worst.items():
        _WORST[f"{form}/{prec}/{k}"] = max(v, _WORST.get(f"{form}/{prec}/{k}", 0.0))


@pytest.mark.parametrize("B,ifam", PER_STAGE, ids=[f"{b}-{f}" for b, f in PER_STAGE])
@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_backward_stages_one_launch_per_stage(prec, B, ifam):
    _note("per-stage", prec, check_step(prec, B, ifam, BF if prec == "bf16" else W, "per-stage"))


def _in_child(env, cases, form, enc_path=None):
    """check_step for every case in a child process with `env`; enc_path: bits giga_encoder_last_path() must report after
    the last case (its training forward)."""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import test_gpu_bwd_stages as T\n"
            "for prec, B, ifam, path in %r:\n"
            "    T.check_step(prec, B, ifam, path, %r)\n"
            "enc = T._capi.lib().giga_encoder_last_path()\n"
            "print('ENCODER PATH', enc)\n"
            "assert %r is None or enc & %r == %r, enc\n"
            "print('ok')\n") % (ROOT, os.path.join(ROOT, "tests"), cases, form, enc_path, enc_path, enc_path)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    print(r.stdout[-12000:])
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count("STAGES ") == len(cases)


def test_backward_stages_direct_dgrad_convolutions():
    """GIGA_WINOGRAD_BWD=0: the fp32 data gradients of the 3x3 layers on the direct kernels."""
    _in_child({"GIGA_WINOGRAD_BWD": "0"}, [("fp32", B, f, 0) for B, f in DIRECT], "direct")


def test_retired_switches_are_not_read():
    """Every removed environment switch at its former non-default value (RETIRED): the 8-scene bf16 step -- 24 images, the size
    from which one of them moved the data-gradient chain into a persistent launch and another kept the forward on per-layer
    launches -- runs one launch per stage on bf16 operands (BWD_PATH_BF16 alone) behind a persistent forward, within the
    per-stage tolerances."""
    _in_child(RETIRED, [("bf16", 8, "uniform", BF)], "retired-switches", enc_path=_capi.PATH_PERSISTENT)
