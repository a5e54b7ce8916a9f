"""GPU: the fp32 training decoder (csrc/giga_decoder_bwd.hip: decoder_bwd_kernel, linear_wgrad_kernel, plane_gather_kernel, launched by
launch_decoder_backward) held BIT FOR BIT to its reference on data where fp32 arithmetic is exact, regime by regime of the launch.

It is the default training path and the reference step of the bf16 one, and the other tests see it only through whole-step parameter
gradients at statistical tolerances (tests/test_gpu_training.py: 2e-3 of a tensor's maximum; tests/test_gpu_backward_envelope.py:
1.25e-4): one query of 4096 dropped from the gather, or one point of 67 551 missing from a weight gradient, passes those.  On the data of
tests/dect_exact.py under precision "fp32" every sum is exact in any order (tests/test_dect_exact_host.py proves it on the CPU,
bounding the sums of absolute values too, and shows that nine defects of this launch each change a compared value), so the comparison
is `==`:
  bit for bit   raw outputs of all four heads (post = 0); the training call's `width` and occupancy outputs; every parameter gradient
                of decoder_qual (sigmoid' = 1/4: the harness hands the backward q = 0.5), decoder_width and decoder_tsdf; every
                parameter gradient of decoder_rot == 0; the plane gradients [3][B][40][40][32] at offset 0 of the backward's
                workspace, as numbers (-0 == 0); and a second run of the same calls returns the same bytes.
  bounded       the gradient of fc_p.weight in point families B and C only: whole-pixel coordinates have 24 significant bits, the
                products G_i p_i are rounded, so it is held to the float64 sum within the worst case of an fp32 sum,
                2 P 2^-23 max_i |G_i p_i| per element (dect_exact.fcp_bound: derived, not measured).
                Measured on an MI355X, worst error / bound over the 16 cases of families B and C: 0.20 (decoder_width at 2 x 1
                grasp points: error 2.4e-7, bound 1.7e-6), 0.15 and 0.14 in the other calls of at most ten points, at most 0.09
                from 33 points up and 0.001 ... 0.011 for the occupancy head (largest error 1.2e-4 where the bound is 0.23, at
                33 x 2047 points); 0 in the one-point case.  These sums go through linear_wgrad_kernel's atomics, so a second run
                may return other bytes for them, within the same bound; every exact value returns the same bytes.
The cases are dect_exact.CASES32: the twelve of dect_exact.CASES in families A and B (one valid lane; idle waves; both routes of the
plane gradient on both sides of 256 and 4096 queries; exactly one persistent round; ragged second rounds; giga_aff, giga_geo,
giga_detach), and 7-32-340-0 (A, B: 85 batches x 3 heads = 255 workgroups, the last shape with one workgroup per head), 7-32-341-0
(A, B: 258 > 256, one workgroup walks three heads), 8-2-0-4096 (A, C: the gather at its upper bound; C has 64 cells of more than 32
points per plane and scene, two more than plane_gather_kernel ranks with the whole workgroup) and 8-2-0-4097 (C: one past it,
atomics).  None is left out.

Exact data cannot see the ORDER of a sum.  test_gathered_plane_gradient_is_reproducible_on_real_data holds what the sorted cell lists
are for: on real-valued planes and gradients two runs of the gathered plane gradient are the same bytes, and it is the float64 sum
of the reference's dc rows to 1e-5 of its maximum.  Measured: 2.2e-7 of the maximum at 2 x 600 whole-pixel points, 2.4e-7 at
2 x 4096 points of family C, 4.0e-6 with the 4096 points of a scene in one cell (one fp32 sum of 4096 terms per pixel)."""
import os
import sys

import pytest
import torch

from giga_amd import synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_exact as X  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("cf", X.CASES32, ids=X.case32_id)
def test_fp32_decoder_is_exact_on_exact_data(cf):
    case, fam = cf
    hp, detach, B, N, M = case
    d = X.data(case, fam, "fp32")
    ref = X.reference(case, fam, "fp32")
    x = torch.from_numpy(synth.tsdf_batch(500, B))
    runs = [X.run_decoder(X.state_dict(fam), hp, detach, x, d["pos"], d["pos_occ"], d["douts"], planes=d["planes"], precision="fp32")
            for _ in range(2)]
    got = runs[0]
    assert torch.equal(got["planes"], d["planes"])           # the decoders did sample the test's planes
    for k, bound in ref.bounds.items():
        err = (got[k].double() - ref.values[k].double()).abs()
        print(f"{X.case32_id(cf)} {k}: worst error {float(err.max()):.3e}, bound there "
              f"{float(bound.flatten()[err.argmax()]):.3e}, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert X.mismatches(got, ref) == []
    assert sorted(k for k in got if k.startswith("grad/")) == sorted(k for k in ref.values if k.startswith("grad/"))
    for k, v in got.items():                                 # `rot`: a zero upstream gradient
        if k.startswith("grad/decoder_rot"):
            assert not bool((v != 0).any()), k
    assert X.mismatches(runs[1], ref) == []
    for k in got:
        # (fc_p.weight in families B and C is a sum of ROUNDED products that linear_wgrad_kernel's blocks add with atomics, in
        # any order: both runs are within the bound, above; their bytes may differ.  Every exact value must not.)
        assert k in ref.bounds or _same_bytes(got[k], runs[1][k]), ("second run differs", k)


def _real_points(kind, B, M, g):
    if kind == "one cell":                                   # every query of a scene inside one pixel cell: one list of M points
        return torch.tensor([0.1013, -0.2031, 0.3047]) + 1e-3 * torch.rand(B, M, 3, generator=g)
    pixels = sorted(X.dec_point.BOUNDARY) if kind == "B" else X.FAMILY_C_PIXELS
    vals = torch.tensor([X.dec_point.BOUNDARY[k] for k in pixels], dtype=torch.float32)
    return vals[torch.randint(0, len(vals), (B, M, 3), generator=g)]


@pytest.mark.parametrize("B,M,kind", [(2, 600, "B"), (2, 4096, "C"), (2, 4096, "one cell")], ids=lambda v: str(v).replace(" ", "-"))
def test_gathered_plane_gradient_is_reproducible_on_real_data(B, M, kind):
    g = torch.Generator().manual_seed(11)
    sd = weights.make_state_dict(7)
    planes = torch.randn(3, B, X.RES, X.RES, X.CD, generator=g)
    pos_occ = _real_points(kind, B, M, g)
    dout = torch.randn(B, M, generator=g)
    assert X.bwd32_calls((8, False, B, 0, M))["occ"]["gather"]
    x = torch.from_numpy(synth.tsdf_batch(500, B))
    runs = [X.run_decoder(sd, 8, False, x, torch.zeros(B, 0, 3), pos_occ, {"decoder_tsdf": dout}, planes=planes, precision="fp32")
            for _ in range(2)]
    assert _same_bytes(runs[0]["gplanes"], runs[1]["gplanes"])                   # the gather sums in a fixed order
    ref = X.occ_plane_grad64(sd, planes, pos_occ, dout)
    err = float((runs[0]["gplanes"].double() - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"{B} x {M} {kind}: worst error {err:.3e} = {err / scale:.3e} of max |ref| {scale:.3e}")
    assert bool(torch.isfinite(runs[0]["gplanes"]).all())
    assert err <= 1e-5 * scale
