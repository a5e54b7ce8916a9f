"""What is planned is what runs: for the smallest shapes that reach each regime of the training decoder's backward, in both
precisions, the first `launches` kernel launches of one giga_backward call carry the kernel names convonet.decoder_backward_plan
(csrc/giga_dec_bwd_plan.h) lists, in its order (the library's launch probe names one launch per call, so the call is repeated on
the same buffers once per planned launch).  The fields a case is about are also written out by hand, so the test fails when the
policy moves as well as when launch and plan part."""
import os
import sys

import pytest
import torch

from giga_amd import _capi, convonet, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_exact as X  # noqa: E402

pytestmark = pytest.mark.gpu
# (head set, detach, B, N, M), the fields of the fp32 plan the case is about
CASES = [
    ((15, False, 1, 1, 1), dict(grasp=dict(grid_y=3, heads_per_wg=1, wgrad_merged=True, nb_total=81), occ=dict(gather=False))),
    ((8, False, 1, 0, 256), dict(occ=dict(gather=True), clear_planes=False)),                 # first gathered size
    ((15, True, 1, 1, 256), dict(occ=dict(gather=False, planes=False), clear_planes=True)),   # detached: no gather
    ((7, False, 32, 341, 0), dict(grasp=dict(nbatch=86, grid_y=1, heads_per_wg=3))),           # one workgroup walks three heads
    ((8, False, 1, 0, 4097), dict(occ=dict(gather=False), clear_planes=True)),                 # one past the gather's bound
]


@pytest.fixture(scope="module")
def events():
    L = _capi.lib()
    ev = (L.giga_event_create(), L.giga_event_create())
    yield ev
    L.giga_event_destroy(ev[0])
    L.giga_event_destroy(ev[1])


@pytest.mark.parametrize("precision", X.PRECISIONS)
@pytest.mark.parametrize("case,fields", CASES, ids=[X.case_id(c) for c, _ in CASES])
def test_planned_launches_are_the_ones_enqueued(events, case, fields, precision):
    hp, detach, B, N, M = case
    L = _capi.lib()
    flags = hp | (_capi.DETACH_OCC if detach else 0) | (_capi.BF16_DECODER if precision == "bf16" else 0)
    plan = convonet.decoder_backward_plan(B, N, M, flags)
    if precision == "fp32":
        for k, want in fields.items():
            got = {f: plan[k][f] for f in want} if isinstance(want, dict) else plan[k]
            assert got == want, (k, plan)
    assert plan["launches"] == len(plan["order"]) >= 2
    g = torch.Generator().manual_seed(B + N + M)
    pos, pos_occ = torch.rand(B, N, 3, generator=g) - 0.5, torch.rand(B, M, 3, generator=g) - 0.5
    douts = {"decoder_qual": torch.randn(B, N, generator=g), "decoder_rot": torch.randn(B, N, 4, generator=g),
             "decoder_width": torch.randn(B, N, generator=g), "decoder_tsdf": torch.randn(B, M, generator=g)}
    names, counts = [], []

    def probe_each_launch(backward):
        for k in range(plan["launches"]):
            before = L.giga_launch_count()
            L.giga_launch_probe(before + 1 + k, events[0], events[1])     # the decoder part is giga_backward's first
            try:
                backward()
                names.append((L.giga_launch_probe_name() or b"").decode())
            finally:
                L.giga_launch_probe(0, None, None)
            counts.append(L.giga_launch_count() - before)

    res = X.run_decoder(weights.make_state_dict(7), hp, detach, torch.from_numpy(synth.tsdf_batch(500, B)), pos, pos_occ, douts,
                        precision=precision, around_backward=probe_each_launch)
    assert len(names) == plan["launches"] and all(want in got for want, got in zip(plan["order"], names)), (plan["order"], names)
    assert len(set(counts)) == 1 and counts[0] > plan["launches"]          # (the encoder's backward follows)
    assert all(bool(torch.isfinite(v).all()) for v in res.values())
