"""CPU tests of the training decoder's backward plan (csrc/giga_dec_bwd_plan.h) through giga_decoder_backward_plan /
convonet.decoder_backward_plan: host only, the built library and no device.  giga_backward launches what this plan says
(tests/test_gpu_decoder_bwd_plan.py holds it to that on the device) and carves its scratch where the plan says, so each threshold of
the policy is pinned here from both sides with the figures of the code as it stands, the regions of every call are shown to lie
inside the step's scratch without overlapping, and giga_backward_workspace_bytes is held to the sizes it returned before the plan
existed."""
import ctypes
import os
import sys

import pytest

from giga_amd import _capi
from giga_amd.convonet import _PLAN_WORDS, decoder_backward_plan

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_exact as X  # noqa: E402

BF16, DETACH = _capi.BF16_DECODER, _capi.DETACH_OCC
ALL_CASES = list(X.CASES) + [c for c, _ in X.CASES32_NEW]


def fp32_call(P, nheads):
    return decoder_backward_plan(1, P, 0, (1 << nheads) - 1)["grasp"]


def test_arguments():
    """The codes giga_backward gives for the same arguments; no scenes: all words zero."""
    L = _capi.lib()
    w = (ctypes.c_int32 * _PLAN_WORDS)()
    assert L.giga_decoder_backward_plan(1, 1, 1, 15, None) == -1
    assert L.giga_decoder_backward_plan(1, -1, 1, 15, w) == -1 and L.giga_decoder_backward_plan(1, 1, -1, 15, w) == -1
    assert L.giga_decoder_backward_plan(3073, 1, 1, 15, w) == -7 and L.giga_decoder_backward_plan(3072, 1, 1, 15, w) == 0
    for B in (0, -1):
        w[0] = 7
        assert L.giga_decoder_backward_plan(B, 5, 5, 15 | BF16, w) == 0 and not any(w)
    d = decoder_backward_plan(2, 0, 0, 15)
    assert not d["occ"]["runs"] and not d["grasp"]["runs"] and d["launches"] == 0 and d["order"] == [] and d["scratch_floats"] == 0
    assert d["clear_planes"] and not d["reduce"]
    # flag bits other than the two the plan reads change nothing
    assert decoder_backward_plan(2, 3, 300, 15 | _capi.BF16_CONVS | _capi.CONVIN_MASK_BWD) == decoder_backward_plan(2, 3, 300, 15)


def test_three_heads_share_a_workgroup_from_86_batches():
    """grid_x * nheads <= 256: 85 batches x 3 = 255 keep one workgroup per head, 86 x 3 = 258 do not."""
    below, at = fp32_call(32 * 340, 3), fp32_call(32 * 341, 3)
    assert (below["nbatch"], below["grid_x"], below["grid_y"], below["heads_per_wg"]) == (85, 85, 3, 1)
    assert (at["nbatch"], at["grid_x"], at["grid_y"], at["heads_per_wg"]) == (86, 86, 1, 3)
    assert (below["block"], below["lds"], below["kernel"]) == (256, 111 * 1024, "decoder_bwd_kernel")
    one = fp32_call(32 * 4 * 300, 1)                          # one head: 300 batches on 256 workgroups, still "split"
    assert (one["nbatch"], one["grid_x"], one["grid_y"], one["heads_per_wg"]) == (300, 256, 1, 1)


def test_gather_bounds():
    """One head, 256 .. 4096 queries per scene, attached: gathered and written; else atomics into a cleared buffer."""
    for prec in (0, BF16):
        got = {M: decoder_backward_plan(2, 0, M, 8 | prec) for M in (255, 256, 4096, 4097)}
        assert [got[M]["occ"]["gather"] for M in (255, 256, 4096, 4097)] == [False, True, True, False]
        assert [got[M]["clear_planes"] for M in (255, 256, 4096, 4097)] == [True, False, False, True]
        det = decoder_backward_plan(2, 1, 256, 15 | DETACH | prec)
        assert not det["occ"]["gather"] and not det["occ"]["planes"] and det["clear_planes"] and det["grasp"]["planes"]
        # the grasp call never gathers, and no call of several heads does
        for nh in (1, 2, 3):
            assert not decoder_backward_plan(2, 256, 0, (1 << nh) - 1 | prec)["grasp"]["gather"]
        assert not decoder_backward_plan(2, 300, 300, 15 | prec)["grasp"]["gather"]


def test_weight_gradient_launches():
    """27 column blocks per head; two or three heads share one launch of 54 / 81."""
    got = {nh: fp32_call(100, nh) for nh in (1, 2, 3)}
    assert [got[nh]["nb_total"] for nh in (1, 2, 3)] == [27, 54, 81]
    assert [got[nh]["wgrad_launches"] for nh in (1, 2, 3)] == [1, 1, 1]
    assert [got[nh]["wgrad_merged"] for nh in (1, 2, 3)] == [False, True, True]
    assert [got[nh]["ksplit_cap"] for nh in (1, 2, 3)] == [75, 37, 25]
    assert [got[nh]["launches"] for nh in (1, 2, 3)] == [2, 2, 2]


@pytest.mark.parametrize("P,nh,ksplit,ppb", [(1, 1, 1, 32), (33, 1, 2, 32), (4200, 1, 66, 64), (65536, 1, 74, 896),
                                              (1, 3, 1, 32), (33, 3, 2, 32), (4200, 3, 22, 192), (65536, 3, 25, 2624)])
def test_split_over_points(P, nh, ksplit, ppb):
    c = fp32_call(P, nh)
    assert (c["ksplit"], c["pts_per_block"]) == (ksplit, ppb)
    assert (c["ksplit"] - 1) * c["pts_per_block"] < P <= c["ksplit"] * c["pts_per_block"] and c["ksplit"] <= c["ksplit_cap"]


@pytest.mark.parametrize("tiles,grid,fwd", [(1, 1, 1), (4, 1, 1), (5, 2, 1), (1024, 256, 128), (1025, 256, 129)])
def test_bf16_grids(tiles, grid, fwd):
    c = decoder_backward_plan(1, 32 * tiles, 0, 7 | BF16)["grasp"]
    assert (c["tiles"], c["grid_x"], c["grid_y"], c["block"], c["lds"], c["kernel"]) == (tiles, grid, 3, 256, 153600, "dect_kernel")
    assert (c["fwd_grid_x"], c["fwd_block"], c["fwd_lds"]) == (fwd, 512, 129024)
    assert c["launches"] == 1 and c["wgrad_launches"] == 0 and c["head_stride"] == grid * 31 * 1024


def test_launch_order():
    fp = decoder_backward_plan(1, 1, 256, 15)
    assert fp["order"] == ["decoder_bwd_kernel", "plane_gather_kernel", "linear_wgrad_kernel", "decoder_bwd_kernel",
                           "linear_wgrad_kernel"] and fp["launches"] == 5 and not fp["reduce"]
    bf = decoder_backward_plan(1, 1, 256, 15 | BF16)
    assert bf["order"] == ["dect_kernel", "plane_gather_kernel", "dect_kernel", "dect_reduce_kernel"] and bf["reduce"]
    assert decoder_backward_plan(1, 1, 255, 15 | BF16)["order"] == ["dect_kernel", "dect_kernel", "dect_reduce_kernel"]
    assert decoder_backward_plan(1, 1, 0, 15)["order"] == ["decoder_bwd_kernel", "linear_wgrad_kernel"]


def _regions(call, base):
    """[(name, first float, one past the last)] of a call's regions, from the step's decoder scratch."""
    P, out = call["P"], []
    per_head = call["head_stride"]
    for k in range(call["nheads"]):
        out.append((f"head{k}", call["head_off"] + k * per_head, call["head_off"] + (k + 1) * per_head))
    for name, width in (("cbuf", 96), ("pbuf", 32), ("dcbuf", 96)):
        if call[name + "_off"] >= 0:
            out.append((name, call[name + "_off"], call[name + "_off"] + P * width))
    assert max(hi for _, _, hi in out) == call["scratch_floats"]
    return [(n, base + lo, base + hi) for n, lo, hi in out]


@pytest.mark.parametrize("prec", (0, BF16), ids=("fp32", "bf16"))
@pytest.mark.parametrize("case", ALL_CASES, ids=X.case_id)
def test_regions_lie_inside_the_scratch_and_apart(case, prec):
    hp, detach, B, N, M = case
    plan = decoder_backward_plan(B, N, M, hp | prec | (DETACH if detach else 0))
    regions = []
    for name in ("occ", "grasp"):
        c = plan[name]
        if not c["runs"]:
            assert c["scratch_floats"] == 0
            continue
        if prec:                                             # bf16: the partial tiles of a head, [grid_x][31][1024]
            assert c["head_stride"] == c["grid_x"] * 31 * 1024 and c["cbuf_off"] == c["pbuf_off"] == -1
            assert (c["dcbuf_off"] >= 0) == (name == "occ")
        else:                                                # fp32: 23 row arrays [P][32] per head
            assert c["head_stride"] == c["P"] * 32 * 23 and min(c["cbuf_off"], c["pbuf_off"], c["dcbuf_off"]) >= 0
        assert not c["gather"] or c["dcbuf_off"] >= 0
        regions += [(name + "." + n, lo, hi) for n, lo, hi in _regions(c, plan[name + "_base"])]
    assert regions
    regions.sort(key=lambda r: r[1])
    assert regions[0][1] >= 0 and regions[-1][2] <= plan["scratch_floats"]
    for (n0, _, hi0), (n1, lo1, _) in zip(regions, regions[1:]):
        assert hi0 <= lo1, (n0, n1)                          # sorted by start: no two regions overlap, within a call or across
    # the step's scratch fits what the size call reserves (it does not know the precision: the larger of the two)
    L = _capi.lib()
    fixed = L.giga_backward_workspace_bytes(B, 0, 0, 0)      # plane gradients + the encoder's share
    assert fixed + 4 * plan["scratch_floats"] <= L.giga_backward_workspace_bytes(B, N, M, hp)


# giga_backward_workspace_bytes(B, N, M, head set) of the commit before the plan (one build of it, asked once), for ALL_CASES
WORKSPACE_BYTES = {
    (15, 1, 1, 1): 452865536,
    (15, 1, 33, 255): 453657344,
    (15, 3, 43, 256): 471296512,
    (15, 7, 3, 600): 512895488,
    (15, 2, 1, 4097): 491209216,
    (15, 16, 1, 2048): 688857088,
    (15, 17, 37, 2047): 709987072,
    (15, 32, 1, 2048): 932724736,
    (15, 33, 1, 2047): 947839744,
    (7, 5, 2, 0): 482208768,
    (8, 3, 0, 300): 470548480,
    (15, 4, 1, 256): 478431232,
    (7, 32, 340, 0): 786595840,
    (7, 32, 341, 0): 786907136,
    (8, 2, 0, 4096): 491182080,
    (8, 2, 0, 4097): 491189760,
}


@pytest.mark.parametrize("case", ALL_CASES, ids=X.case_id)
def test_workspace_bytes_are_the_earlier_ones(case):
    hp, detach, B, N, M = case
    L = _capi.lib()
    assert L.giga_backward_workspace_bytes(B, N, M, hp) == WORKSPACE_BYTES[hp, B, N, M]
    assert L.giga_backward_workspace_bytes(B, N, M, hp | DETACH | BF16) == WORKSPACE_BYTES[hp, B, N, M]     # (flag bits are masked)
