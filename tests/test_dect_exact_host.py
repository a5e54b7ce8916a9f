"""CPU: the exact data of tests/dect_exact.py IS exact, and it sees the faults it is meant for.

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
        if k.startswith("grad/") and head in X.EXACT_HEADS:
            assert bool((v != 0).any()), k
            if k.endswith(".weight"):
                dens = float((v != 0).float().mean())
                least = min(least, (dens, k))
                assert dens >= (ONE_POINT if ref.heads[head]["P"] == 1 else 0.10), (k, dens)
        if k.startswith("grad/") and head not in X.EXACT_HEADS:
            assert not bool((v != 0).any()), k               # zero upstream gradient: exactly zero
    assert bool((ref.values["gplanes"] != 0).any())
    for h in ref.heads:
        if h in X.EXACT_HEADS:
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
    """Points of workgroup nwg - 1 under the kernel's tile_lo / tile_hi split (dect_kernel, dect_grid)."""
    tiles = (P + 31) // 32
    nwg = min((tiles + 3) // 4, 256)
    return torch.arange(32 * (tiles * (nwg - 1) // nwg), P)


@pytest.mark.parametrize("fam", X.FAMILIES)
@pytest.mark.parametrize("case", SENSITIVITY_CASES, ids=X.case_id)
def test_the_data_sees_each_defect(case, fam):
    hp, detach, B, N, M = case
    ref = X.reference(case, fam)
    assert X.mismatches(ref.values, ref) == []
    heads = [h for h in X.EXACT_HEADS if h in ref.heads]

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
