"""CPU: the exact data of tests/dect_exact.py IS exact, and it sees the faults it is meant for (bf16 first, fp32 below).

For every case of dect_exact.CASES and both point families the operand-rounded reference (tests/dect_ref.py, float64 sums) rounds
no operand, every output and gradient is a multiple of 1/4 below 2^22 (so fp32 holds every sum, in any order), every gradient
tensor of the `width` and occupancy heads has a nonzero entry and every weight-gradient matrix at least 10 % of them.  The
sensitivity check applies six defects a kernel could have to the REFERENCE's result and asserts that the comparison the GPU test
makes (dect_exact.mismatches) reports each.  No kernel runs here."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_exact as X  # noqa: E402
import ref64  # noqa: E402
from giga_amd import _capi, convonet  # noqa: E402


# A call of ONE point has rank-one weight gradients dY (x) X, whose density is the product of the two vectors' densities: dY of
# blocks.4.fc_1 has at most the eight entries of fc_out's row (25 %) and X, a ReLU output, about half of its 32, and in every other
# layer both factors are ReLU-masked.  No seed reaches 10 % there (40 000 per family tried: at most 8.8 %); a quarter of a quarter
# -- both factors a quarter dense -- is asked instead, and only of the (1, 1, 1) case.  Every call of two points or more holds 10 %.
ONE_POINT = 1.0 / 16


@pytest.mark.parametrize("fam", X.FAMILIES)
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_the_data_is_exact(case, fam):
    ref = X.reference(case, fam)
    changed = {h: v["stat"]["changed"] for h, v in ref.heads.items()}
    biggest = max(v["stat"]["max"] for v in ref.heads.values())
    assert all(v["stat"]["calls"] > 40 for v in ref.heads.values())          # (the counter did wrap the reference's roundings)
    assert not any(changed.values()), changed
    worst, least = 0.0, (1.0, "")
    for k, v in ref.values.items():
        if k in ref.bounds:                                  # fc_p.weight in family B: the coordinates are no bf16 values
            continue
        q = v.double() * 4.0
        assert bool((q == q.round()).all()), k
        assert float(v.abs().max()) < 2.0 ** 22, (k, float(v.abs().max()))
        worst = max(worst, float(v.abs().max()))
        head = k.split("/")[-1].split(".")[0]
        if k.startswith("grad/") and head in X.EXACT_HEADS["bf16"]:
            assert bool((v != 0).any()), k
            if k.endswith(".weight"):
                dens = float((v != 0).float().mean())
                least = min(least, (dens, k))
                assert dens >= (ONE_POINT if ref.heads[head]["P"] == 1 else 0.10), (k, dens)
        if k.startswith("grad/") and head not in X.EXACT_HEADS["bf16"]:
            assert not bool((v != 0).any()), k               # zero upstream gradient: exactly zero
    assert bool((ref.values["gplanes"] != 0).any())
    for h in ref.heads:
        if h in X.EXACT_HEADS["bf16"]:
            assert float(X.data(case, fam)["douts"][h][-1, -1]) != 0.0      # the point the kernel pads idle lanes with
    print(f"{X.case_id(case)} {fam}: 0 changed operands, max |operand| {biggest}, max |value| {worst}, least dense {least}")


def test_the_sampler_is_the_references_at_the_kernels_pixel_coordinates():
    """dect_exact.sample_features against tests/ref64.py (float64 pixel coordinates) on real-valued planes and uniform points: the
    same operation, 1e-6 apart (an fp32 pixel coordinate is 39 * 2^-24 off); and whole pixels of family B take ONE tap."""
    g = torch.Generator().manual_seed(1)
    planes = {k: torch.randn(2, 32, 40, 40, generator=g, dtype=torch.float64) for k in X.O.PLANES}
    p = torch.rand(2, 500, 3, generator=g) * 1.3 - 0.65
    assert float((X.sample_features(p, planes) - ref64.sample_features(p, planes)).abs().max()) < 2e-5
    pb = X.data(X.CASES[2], "B")["pos_occ"]
    f = X.pix_coord(X.O.normalize_coordinate(pb, "xz"))
    assert bool((f == f.round()).all()) and float(f.max()) <= 38.0 and float(f.min()) == 0.0


SENSITIVITY_CASES = [X.CASES[2], X.CASES[3], X.CASES[11]]   # 129 ragged points on 2 workgroups; 33 workgroups; the detached model


def _last_workgroup(P):
    """Points of workgroup nwg - 1 under the kernel's tile_lo / tile_hi split (dect_kernel), nwg the bf16 call's grid_x in the
    library's plan."""
    call = convonet.decoder_backward_plan(1, P, 0, 1 | _capi.BF16_DECODER)["grasp"]
    tiles, nwg = call["tiles"], call["grid_x"]
    return torch.arange(32 * (tiles * (nwg - 1) // nwg), P)


@pytest.mark.parametrize("fam", X.FAMILIES)
@pytest.mark.parametrize("case", SENSITIVITY_CASES, ids=X.case_id)
def test_the_data_sees_each_defect(case, fam):
    hp, detach, B, N, M = case
    ref = X.reference(case, fam)
    assert X.mismatches(ref.values, ref) == []
    heads = [h for h in X.EXACT_HEADS["bf16"] if h in ref.heads]

    def with_grads(fn):
        got = dict(ref.values)
        for h in heads:
            for k, v in fn(h).items():
                got[k] = v
        return got

    def seen(got, what, only=None):
        bad = X.mismatches(got, ref)
        assert bad, what
        if only is not None:
            assert all(only(b[0]) for b in bad), (what, bad)
        return bad

    weight_grad = lambda k: k.startswith("grad/")  # noqa: E731
    # 1. the last point of a call (what idle lanes are padded with) once more in every weight gradient
    def once_more(h):
        P = ref.heads[h]["P"]
        extra = ref.head_grads(h, torch.tensor([P - 1]))
        return {k: ref.values[k] + v for k, v in extra.items()}
    bad = seen(with_grads(once_more), "padding leak", weight_grad)
    assert {b[0].split("/")[1].split(".")[0] for b in bad} == set(heads)
    # 2. the last workgroup's partial image dropped by the reduce
    def dropped(h):
        gone = ref.head_grads(h, _last_workgroup(ref.heads[h]["P"]))
        return {k: ref.values[k] - v for k, v in gone.items()}
    bad = seen(with_grads(dropped), "dropped partial image", weight_grad)
    assert {b[0].split("/")[1].split(".")[0] for b in bad} == set(heads)
    # 3. fc_p.weight's gradient without its p_lo term (family B: the coordinates have one)
    if fam == "B":
        def no_lo(h):
            s = ref.heads[h]["saved"]
            k = f"grad/{h}.fc_p.weight"
            return {k: (s["dn0"].double().T @ s["p_hi"].double()).float().reshape(ref.values[k].shape)}
        bad = seen(with_grads(no_lo), "p_lo dropped", lambda k: k.endswith("fc_p.weight"))
        assert len(bad) == len(heads)
    # 4. a >= ReLU mask in the gradient chain
    seen(with_grads(lambda h: ref.head_grads(h, relu_mask=lambda x: x >= 0)), ">= mask", weight_grad)
    # 5. the occupancy head's plane gradient added although the model detaches it
    det = ref if detach else X.reference((hp, True, B, N, M), fam)
    att = ref if not detach else X.reference((hp, False, B, N, M), fam)
    leaked = det.values["gplanes"] + det.occ_planes
    assert torch.equal(leaked, att.values["gplanes"])
    got = dict(det.values)
    got["gplanes"] = leaked
    bad = X.mismatches(got, det)
    assert [b[0] for b in bad] == ["gplanes"], bad
    # 6. one scene's plane gradient on the next scene
    got = dict(ref.values)
    got["gplanes"] = ref.values["gplanes"].roll(1, dims=1)
    seen(got, "scene shifted", lambda k: k == "gplanes")


# ---- the fp32 training decoder (csrc/giga_decoder_bwd.hip) ------------------------------------------------------------------------
# The same data under precision "fp32": the chain of tests/dect_ref.py with no rounding, `qual` with a gradient (dO = d / 4), point
# family C.  Beyond the final values, the sums of ABSOLUTE values that dominate every partial sum are bounded, so that exactness holds
# for any order of summation -- decoder_bwd_kernel's atomics, linear_wgrad_kernel's split over points and waves, the gather.
def _quantum(t):
    """The largest 2^-k of which every entry of t is a whole multiple."""
    for k in range(0, 24):
        u = t.double() * 2.0 ** k
        if bool((u == u.round()).all()):
            return 2.0 ** -k
    raise AssertionError("no dyadic values")


def _dominated(total, quantum, what):
    """Every partial sum of terms that are multiples of `quantum` and whose absolute values sum to `total` is a multiple of
    `quantum` below `total`: fp32 holds it exactly if total / quantum < 2^24.  (The issue's own bound, 2^22, on top.)"""
    assert total < 2.0 ** 22, (what, total)
    assert total / quantum < 2.0 ** 24, (what, total, quantum)


@pytest.mark.parametrize("cf", X.CASES32, ids=X.case32_id)
def test_the_fp32_data_is_exact(cf):
    case, fam = cf
    hp, detach, B, N, M = case
    ref = X.reference(case, fam, "fp32")
    exact = X.EXACT_HEADS["fp32"]
    assert ref.exact_heads == exact and all(v["stat"]["calls"] > 40 for v in ref.heads.values())
    worst, least = 0.0, (1.0, "")
    for k, v in ref.values.items():
        if k in ref.bounds:                                  # fc_p.weight in families B and C: held to fcp_bound, a derived bound
            assert fam != "A" and k.endswith("fc_p.weight") and bool((ref.bounds[k] >= 0).all())
            continue
        q = v.double() * 4.0
        assert bool((q == q.round()).all()), k
        assert float(v.abs().max()) < 2.0 ** 22, (k, float(v.abs().max()))
        worst = max(worst, float(v.abs().max()))
        head = k.split("/")[-1].split(".")[0]
        if k.startswith("grad/") and head in exact:
            assert bool((v != 0).any()), k
            if k.endswith(".weight"):
                dens = float((v != 0).float().mean())
                least = min(least, (dens, k))
                assert dens >= (ONE_POINT if ref.heads[head]["P"] == 1 else 0.10), (k, dens)
        if k.startswith("grad/") and head not in exact:
            assert not bool((v != 0).any()), k               # `rot`: zero upstream gradient, exactly zero
    assert sorted(ref.bounds) == sorted(f"grad/{h}.fc_p.weight" for h in ref.heads if h in exact and fam != "A")
    # the sums that dominate every partial sum
    worst_abs = 0.0
    for h in ref.heads:
        for k, (dY, Xm) in ref.pairs(h).items():
            if k == "fc_p.weight" and fam != "A":            # (whole-pixel coordinates are no short values: ref.bounds)
                continue
            total = dY.abs().T @ Xm.abs() if Xm is not None else dY.abs().sum(0)
            quantum = _quantum(dY) * (_quantum(Xm) if Xm is not None else 1.0)
            _dominated(float(total.max()), quantum, (h, k))
            worst_abs = max(worst_abs, float(total.max()))
    attached = [h for h in ref.heads if not (detach and h == "decoder_tsdf")]
    gp = sum(ref.plane_grad(h) for h in attached) if attached else torch.zeros_like(ref.values["gplanes"]).double()
    assert torch.equal(gp, ref.values["gplanes"].double())   # scatter_planes IS sample_features' backward
    if attached:
        gabs = sum(ref.plane_grad(h, absolute=True) for h in attached)
        wq = min(_quantum(w) for h in attached for k in X.O.PLANES for _, w in X.footprint(ref.heads[h]["p"], k))
        _dominated(float(gabs.max()), wq * min(_quantum(ref.heads[h]["dc"]) for h in attached), "gplanes")
        worst_abs = max(worst_abs, float(gabs.max()))
    assert bool((ref.values["gplanes"] != 0).any()) or not attached
    d = X.data(case, fam, "fp32")
    for h in ref.heads:
        if h in exact:
            assert float(d["douts"][h][-1, -1]) != 0.0      # the point the kernel pads idle lanes with
    if "decoder_qual" in ref.heads:
        assert set(d["douts"]["decoder_qual"].unique().tolist()) <= {-8.0, -4.0, 0.0, 4.0, 8.0}
    # where the rounding reference rounds nothing on this data, the two references are the same numbers
    r16 = X.Reference(case, fam, "bf16", data_of="fp32")
    changed = sum(v["stat"]["changed"] for v in r16.heads.values())
    assert changed == sum(v["stat"]["changed"] for v in ref.heads.values())      # (the fp32 one counts what bf16 WOULD round)
    if changed == 0:
        qual = ref.plane_grad("decoder_qual") if "decoder_qual" in ref.heads else 0.0
        for k, v in r16.values.items():
            if k == "gplanes":
                assert torch.equal(v.double(), ref.values[k].double() - qual), k
            elif k.endswith("fc_p.weight") and fam != "A":   # (p_hi + p_lo is 16 bits of a whole pixel's 24: another sum)
                continue
            elif not k.startswith("grad/decoder_qual"):
                assert torch.equal(v, ref.values[k]), k
    print(f"{X.case32_id(cf)}: max |value| {worst}, max sum of |terms| {worst_abs}, least dense {least}, bf16 would round {changed}")


def _long_cells(p):
    """[plane][scene] -> the cells (o00 of bilin_setup) that hold more than PS_LONG = 32 points, ascending."""
    cells = X.cells(p)
    return [[[c for c, n in enumerate(torch.bincount(cells[i, b], minlength=1600).tolist()) if n > 32]
             for b in range(p.shape[0])] for i in range(3)]


def test_the_fp32_cases_reach_every_launch_regime():
    """With the library's plan (dect_exact.bwd32_calls): the regimes of launch_decoder_backward that the table is for."""
    calls = [(cf, name, L) for cf in X.CASES32 for name, L in X.bwd32_calls(cf[0]).items()]
    several = [L for _, _, L in calls if L["nheads"] > 1]
    assert any(L["split"] for L in several) and any(not L["split"] for L in several)            # both sides of the head split ...
    assert {85, 86} <= {L["nbatch"] for L in several if L["nheads"] == 3}                        # ... at its very threshold
    assert any(L["nbatch"] > 256 and L["nbatch"] % 256 for _, _, L in calls)                     # a ragged second round
    assert any(L["ksplit"] < L["ksplit_cap"] for _, _, L in calls)
    assert any(L["ksplit"] > 1 and L["last_block"] % 8 for _, _, L in calls)
    assert any(L["last_block"] < L["pts_per_block"] and L["ksplit"] > 1 for _, _, L in calls)
    assert any(L["P"] < 8 for _, _, L in calls)
    assert any(L["nb_total"] == 27 for _, _, L in calls) and any(L["nb_total"] == 81 for _, _, L in calls)
    per_scene = {cf[0][4]: L["gather"] for cf, name, L in calls if name == "occ" and not cf[0][1]}
    assert {255, 256, 4096, 4097} <= set(per_scene)
    assert [per_scene[m] for m in (255, 256, 4096, 4097)] == [False, True, True, False]
    assert any(cf[0][1] and name == "occ" and not L["gather"] for cf, name, L in calls)          # (detached: no gather)
    fams_c = [cf for cf in X.CASES32 if cf[1] == "C"]
    assert {cf[0][4] for cf in fams_c} == {4096, 4097}
    for case, fam in fams_c:
        for per_plane in _long_cells(X.data(case, fam, "fp32")["pos_occ"]):
            for long in per_plane:
                assert len(long) >= 63, (case, len(long))    # more than plane_gather_kernel lists (62): the serial fall-back runs


SENSITIVITY32 = [(X.CASES[2], "A"), (X.CASES[2], "B"), (X.CASES[11], "B"), (X.CASES[6], "A"), ((8, False, 2, 0, 4096), "C")]
DEFECTS32 = ("padding leak", ">= mask", "detached occupancy leak", "scene shift", "last ksplit block", "bias from wave 0",
             "width's plane share", "second round", "long cells beyond 62")


def _applicable32(case, fam):
    hp, detach, B, N, M = case
    calls = X.bwd32_calls(case)
    names = {"padding leak", ">= mask"}
    if hp & 8 and M > 0:
        names.add("detached occupancy leak")
    if B > 1:
        names.add("scene shift")
    if any(L["ksplit"] > 1 for L in calls.values()):
        names.add("last ksplit block")
    if any(L["P"] > 8 for L in calls.values()):
        names.add("bias from wave 0")
    if hp & 4 and "grasp" in calls and calls["grasp"]["nheads"] > 1 and calls["grasp"]["split"]:
        names.add("width's plane share")
    if any(L["round2"] for L in calls.values()):
        names.add("second round")
    if fam == "C" and calls.get("occ", {}).get("gather"):
        names.add("long cells beyond 62")
    return names


def test_every_fp32_defect_has_a_case():
    assert set().union(*(_applicable32(c, f) for c, f in SENSITIVITY32)) == set(DEFECTS32)
    assert all(cf in X.CASES32 for cf in SENSITIVITY32)


@pytest.mark.parametrize("cf", SENSITIVITY32, ids=X.case32_id)
def test_the_fp32_data_sees_each_defect(cf):
    """Each defect is applied to the REFERENCE's result; dect_exact.mismatches, the GPU test's comparison, must report it."""
    case, fam = cf
    hp, detach, B, N, M = case
    ref = X.reference(case, fam, "fp32")
    assert X.mismatches(ref.values, ref) == []
    heads = [h for h in X.EXACT_HEADS["fp32"] if h in ref.heads]
    calls = X.bwd32_calls(case)
    call_of = lambda h: calls["occ" if h == "decoder_tsdf" else "grasp"]  # noqa: E731
    todo = _applicable32(case, fam)
    done = set()

    def with_grads(fn, base=None):
        got = dict(base if base is not None else ref.values)
        for h in heads:
            for k, v in fn(h).items():
                got[k] = v
        return got

    def seen(got, what, only=None, every_head=False):
        bad = X.mismatches(got, ref)
        assert bad, what
        if only is not None:
            assert all(only(b[0]) for b in bad), (what, bad)
        if every_head:
            assert {b[0].split("/")[1].split(".")[0] for b in bad if b[0].startswith("grad/")} == set(heads), (what, bad)
        done.add(what)

    def without(h, idx, keys=lambda k: True):
        if len(idx) == 0:
            return {}
        return {k: ref.values[k] - v for k, v in ref.head_grads(h, idx).items() if keys(k)}

    weight_grad = lambda k: k.startswith("grad/")  # noqa: E731
    # the last point of a call (what idle lanes are padded with) once more in every weight gradient
    def once_more(h):
        extra = ref.head_grads(h, torch.tensor([ref.heads[h]["P"] - 1]))
        return {k: ref.values[k] + v for k, v in extra.items()}
    seen(with_grads(once_more), "padding leak", weight_grad, every_head=True)
    seen(with_grads(lambda h: ref.head_grads(h, relu_mask=lambda x: x >= 0)), ">= mask", weight_grad)
    if "detached occupancy leak" in todo:
        det = ref if detach else X.reference((hp, True, B, N, M), fam, "fp32")
        att = ref if not detach else X.reference((hp, False, B, N, M), fam, "fp32")
        leaked = det.values["gplanes"] + det.occ_planes
        assert torch.equal(leaked, att.values["gplanes"])
        got = dict(det.values)
        got["gplanes"] = leaked
        assert [b[0] for b in X.mismatches(got, det)] == ["gplanes"]
        done.add("detached occupancy leak")
    if "scene shift" in todo:
        got = dict(ref.values)
        got["gplanes"] = ref.values["gplanes"].roll(1, dims=1)
        seen(got, "scene shift", lambda k: k == "gplanes")
    # linear_wgrad_kernel: the last block of points lost; the bias summed by wave 0 alone (its points: (p - p0) % 32 < 8, p0 the
    # block's first point, a multiple of 32)
    if "last ksplit block" in todo:
        def last_block(h):
            L = call_of(h)
            return without(h, torch.arange((L["ksplit"] - 1) * L["pts_per_block"], L["P"]) if L["ksplit"] > 1 else [])
        seen(with_grads(last_block), "last ksplit block", weight_grad)
    if "bias from wave 0" in todo:
        def wave0(h):
            P = call_of(h)["P"]
            assert call_of(h)["pts_per_block"] % 32 == 0
            idx = torch.arange(P)
            return without(h, idx[idx % 32 >= 8], lambda k: k.endswith(".bias"))
        seen(with_grads(wave0), "bias from wave 0", lambda k: k.endswith(".bias"))
    # decoder_bwd_kernel: one head's workgroups of the split launch lost; the persistent loop's second round lost
    if "width's plane share" in todo:
        got = dict(ref.values)
        got["gplanes"] = (ref.values["gplanes"].double() - ref.plane_grad("decoder_width")).float()
        seen(got, "width's plane share", lambda k: k == "gplanes")
    if "second round" in todo:
        gone = {}
        for h in heads:
            L = call_of(h)
            g = torch.arange(L["P"])
            late = torch.isin(g // 128, torch.tensor(L["round2"], dtype=torch.long))
            assert bool(late.any()) == bool(L["round2"])
            gone[h] = late
        got = with_grads(lambda h: without(h, torch.nonzero(gone[h])[:, 0]))
        gp = ref.values["gplanes"].double()
        for h in heads:
            if gone[h].any() and not (detach and h == "decoder_tsdf"):
                gp = gp - ref.plane_grad(h, keep=gone[h])
        got["gplanes"] = gp.float()
        seen(got, "second round")
        assert "gplanes" in [b[0] for b in X.mismatches(got, ref)]
    # plane_gather_kernel: the cells beyond the 62 long ones it lists lose their points (here: the highest-numbered ones)
    if "long cells beyond 62" in todo:
        p = ref.heads["decoder_tsdf"]["p"]
        cells, long = X.cells(p), _long_cells(p)
        gp = ref.values["gplanes"].double().clone()
        for i in range(3):
            lost = torch.stack([torch.isin(cells[i, b], torch.tensor(long[i][b][62:], dtype=torch.long)) for b in range(B)])
            assert bool(lost.any(dim=1).all())
            gp[i] -= ref.plane_grad("decoder_tsdf", keep=lost.reshape(-1))[i]
        got = dict(ref.values)
        got["gplanes"] = gp.float()
        seen(got, "long cells beyond 62", lambda k: k == "gplanes")
    assert done == todo, (done, todo)
