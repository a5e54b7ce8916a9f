"""CPU checks of the stage-by-stage backward reference (tests/bwd_stage_ref.py) and of the tolerances
tests/test_gpu_bwd_stages.py holds the kernels to.

1. Chained stages equal autograd: every stage reference, fed autograd's gradient of its input, gives autograd's gradient of
   its output to 1e-12 of the range -- both concat halves and both pool stages included, on 'structured' inputs too (their
   constant regions hold pool ties) -- and the three weight / bias references equal autograd's parameter gradients.
2. Discriminating power: each realistic bug, applied to ONE stage on the shapes the GPU test runs, moves some element of that
   stage's output by at least 4x the tolerance of that stage (pool stages are compared bit for bit: any change counts), while
   a correct evaluation in fp32 arithmetic of either form's reference (bf16-rounded operands, or unrounded ones) stays inside."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bwd_stage_ref as R  # noqa: E402
import ref64  # noqa: E402

# (scenes, input family): the shapes and inputs of tests/test_gpu_bwd_stages.py, 'he-7' weights
CASES = [(3, "uniform"), (8, "uniform"), (9, "uniform"), (11, "uniform"), (3, "structured"), (11, "structured")]
_CACHE = {}


def autograd_case(B, ifam):
    """(sd, acts, grads, pgrads) in float64: the U-Net's activations on the three planes of B scenes (3B images), the
    gradient buffers of bwd_stage_ref by autograd for a random upstream gradient, and the U-Net's parameter gradients."""
    if (B, ifam) in _CACHE:
        return _CACHE[B, ifam]
    sd = {k: v.double() for k, v in ref64.weight_family("he-7").items() if k.startswith("encoder.")}
    x = torch.from_numpy(ref64.input_family(ifam, B, first=500)).double()
    with torch.no_grad():
        planes = O.project_planes(O.conv_in_relu(sd, x))
    p0 = torch.cat([planes[k] for k in O.PLANES]).requires_grad_(True)
    sdg = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    cats = []
    cat = torch.cat

    def keeping_cat(ts, dim=0):
        out = cat(ts, dim)
        out.retain_grad()
        cats.append(out)
        return out

    torch.cat = keeping_cat                  # unet_stages concatenates inline: keep the two concatenated inputs' gradients
    try:
        st = O.unet_stages(sdg, p0)
    finally:
        torch.cat = cat
    for t in st.values():
        t.retain_grad()
    gout = torch.randn(st["OUT"].shape, generator=torch.Generator().manual_seed(B), dtype=torch.float64)
    (st["OUT"] * gout).sum().backward()
    acts = {k: v.detach() for k, v in st.items() if k != "OUT"}
    acts["P0"] = p0.detach()
    relu_out = lambda n: st[n].grad * (st[n] > 0)  # noqa: E731  (gradient w.r.t. the pre-activation)
    grads = {"gOUT": gout, "gC0": cats[0].grad, "gC1": cats[1].grad, "gQ1": st["Q1"].grad, "gQ0": st["Q0"].grad, "gP0": p0.grad}
    grads.update({"g" + n: relu_out(n) for n in ("A6", "A5", "A4", "A3", "S2", "A2", "S1", "A1", "S0", "A0")})
    assert set(grads) == set(R.GRAD) and all(tuple(grads[k].shape[1:]) == (c, h, h) for k, (c, h) in R.GRAD.items())
    _CACHE[B, ifam] = (sd, acts, grads, {k: v.grad for k, v in sdg.items()})
    return _CACHE[B, ifam]


@pytest.mark.parametrize("B,ifam", [(3, "uniform"), (3, "structured")])
def test_chained_stages_equal_autograd(B, ifam):
    sd, acts, grads, pgrads = autograd_case(B, ifam)
    if ifam == "structured":                                  # the case is there for its ties: make sure it has them
        s = acts["S1"]
        assert int(((F.max_pool2d(s, 2, 2) > 0) & (R.upsample2(F.max_pool2d(s, 2, 2)) == s).reshape(
            s.shape[0], s.shape[1], 10, 2, 10, 2).sum((3, 5)).gt(1)).sum()) > 100
    for st in R.STAGES:
        want, mag = R.stage_want(st, grads, acts, sd)
        ref = grads[st.dst]
        assert want.dtype == torch.float64 and want.shape == ref.shape, st.name
        err = float((want - ref).abs().max()) / float(ref.max() - ref.min())
        assert err <= 1e-12, (st.name, err)
        assert bool((mag >= want.abs() * (1 - 1e-12)).all()), st.name
    for e in R.WGRADS:
        (dw, mw), (db, mb) = R.wgrad_want(e, grads, acts)
        for got, ref in ((dw, pgrads[R.PREFIX + e[2] + ".weight"]), (db, pgrads[R.PREFIX + e[2] + ".bias"])):
            assert got.shape == ref.shape, e[0]
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.max() - ref.min()), e[0]
        assert bool((mw >= dw.abs() * (1 - 1e-12)).all()) and bool((mb >= db.abs() * (1 - 1e-12)).all())


# ---- discriminating power ------------------------------------------------------------------------------------------------
def _mutant(name, st, grads, acts, sd, r):
    """The output of stage st with one bug, from the same inputs as bwd_stage_ref.stage_want(..., r); None: not applicable."""
    q = r if r is not None else (lambda t: t)
    if st.kind == "pool":
        d, g, s = grads[st.src][:, st.lo:st.hi], R.upsample2(grads[st.dq]), acts[st.mask]
        zero = torch.zeros_like(g)
        if name == "mask_ge":                                 # S >= 0 holds everywhere behind a ReLU
            return d + torch.where(R.first_max(s), g, zero)
        if name == "tie_all":                                 # every element equal to its window's maximum receives dQ
            return torch.where(s > 0, d + torch.where(s == R.upsample2(F.max_pool2d(s, 2, 2)), g, zero), zero)
        return None
    w = sd[R.PREFIX + st.key + ".weight"]
    act = acts[st.mask] if st.mask else None
    if name == "unflipped" and st.kind in ("conv3", "up"):
        return R.conv_stage(st, grads[st.src], w.flip(2, 3), act, r)[0]
    if name == "border_tap" and st.kind == "conv3":           # output row 0 without the tap that reads dY's row 1
        one = torch.zeros_like(w)
        one[:, :, 0, 1] = w[:, :, 0, 1]
        out = R.conv_stage(st._replace(mask=None), grads[st.src], w, None, r)[0]
        out[:, :, 0, :] -= R.conv_stage(st._replace(mask=None), grads[st.src], one, None, r)[0][:, :, 0, :]
        return out * (act > 0) if st.mask else out
    if name == "swap_halves" and st.dst in ("gC1", "gC0"):
        out = R.conv_stage(st, grads[st.src], w, act, r)[0]
        h = out.shape[1] // 2
        return torch.cat((out[:, h:], out[:, :h]), 1)
    if name == "mask_ge" and st.mask:
        return R.conv_stage(st._replace(mask=None), grads[st.src], w, None, r)[0]
    if name == "fp32_operands" and r is not None:
        return R.conv_stage(st, grads[st.src], w, act, None)[0]
    if name == "dy_only" and r is not None:
        return R.conv_stage(st, q(grads[st.src]), w, act, None)[0]
    return None


MUTATIONS = ("unflipped", "border_tap", "swap_halves", "mask_ge", "tie_all", "fp32_operands", "dy_only")
FORMS = {"bf16": (R.bf16, R.tol_bf16), "fp32": (None, R.tol_fp32)}


@pytest.mark.parametrize("B,ifam", CASES, ids=[f"{b}-{f}" for b, f in CASES])
def test_tolerances_reject_one_stage_bugs_by_4x(B, ifam):
    sd, acts, g64, _ = autograd_case(B, ifam)
    grads = {k: v.float().double() for k, v in g64.items()}      # the kernels' buffers are fp32
    table, seen = [], set()
    for form, (r, tol_of) in FORMS.items():
        for st in R.CONV_STAGES:
            want, mag = R.stage_want(st, grads, acts, sd, r)
            tol = tol_of(want, mag)
            # a correct evaluation in fp32 arithmetic (rounded operands are exact in fp32; fp32 products and sums) stays inside
            q = r if r is not None else (lambda t: t)
            w32 = q(sd[R.PREFIX + st.key + ".weight"]).float()
            got32 = R._conv_dgrad(st.kind, q(grads[st.src][:, st.lo:st.hi]).float(), w32).double()
            if st.mask:
                got32 = got32 * (acts[st.mask] > 0)
            inside = float(((got32 - want).abs() / tol).max())
            assert inside <= 1.0, (form, st.name, inside)
            for m in MUTATIONS:
                bad = _mutant(m, st, grads, acts, sd, r)
                if bad is None:
                    continue
                ratio = float(((bad - want).abs() / tol).max())
                table.append((form, st.name, m, ratio))
                seen.add(m)
    for st in R.STAGES:
        if st.kind != "pool":
            continue
        g32 = {k: v.float() for k, v in grads.items()}
        a32 = {k: v.float() for k, v in acts.items()}
        want, _ = R.stage_want(st, g32, a32, sd)
        assert want.dtype == torch.float32
        for m in ("mask_ge", "tie_all"):
            if m == "tie_all" and ifam != "structured":           # uniform noise has no tied windows
                continue
            bad = _mutant(m, st, g32, a32, sd, None)
            d = float((bad - want).abs().max()) / float(want.abs().max())
            # bit-equal is the pool stages' bound: any change counts; the figure is the change relative to the largest element
            table.append(("exact", st.name, m, float("inf") if d > 0 else 0.0))
            seen.add(m)
            assert d >= 4 * 2e-5, (st.name, m, d)
    print(f"\nmutation table B={B} {ifam}: worst change / tolerance")
    for form, name, m, ratio in table:
        print(f"MUT {form:5} {name:5} {m:13} {ratio:10.1f}")
    weak = [t for t in table if not t[3] >= 4.0]
    assert not weak, weak
    assert seen == set(MUTATIONS) - (set() if ifam == "structured" else {"tie_all"}), seen
