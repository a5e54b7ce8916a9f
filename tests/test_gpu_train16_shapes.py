"""GPU: the bf16 training decoder (csrc/giga_decoder_train16.hip: dect_kernel forward and backward, dect_reduce_kernel, both routes of
the plane gradient) held BIT FOR BIT to its reference on data where bf16 arithmetic is exact, shape by shape and model by model.

tests/test_gpu_train16.py compares real-valued data, where two valid bf16 evaluations decorrelate and the bounds are statistical: a
contribution worth a few 1e-3 of a tensor's L2 -- a padded lane, a dropped partial image, the ragged tile of a second round -- passes.
On the data of tests/dect_exact.py no operand is rounded and every sum fits fp32 (tests/test_dect_exact_host.py proves both on the CPU,
and that six such defects each change a compared value), so nothing depends on the summation order, the atomics or the wave that
summed a tile, and the comparison is `==`:
  bit for bit   raw outputs of all four heads (post = 0); the training call's `width` and occupancy outputs; every parameter gradient
                of decoder_width and decoder_tsdf; every parameter gradient of decoder_qual and decoder_rot == 0 (their upstream
                gradients are zero: sigmoid and normalize are not exact); the plane gradients [3][B][40][40][32], as numbers (-0 == 0);
                and a second run of the same calls returns the same bytes.
  bounded       the gradient of fc_p.weight in point family B only: its coordinates (whole pixels in the kernels' fp32 arithmetic)
                are no bf16 values, the kernel multiplies their hi and lo bf16 parts and sums P fp32 terms, so it is held to the
                float64 sum within the worst case of an fp32 sum, 2 P 2^-23 max_i |G_i p_i| per element.  Measured on an MI355X:
                worst error 4.5e-8 where the bound is 6.7e-2 (decoder_tsdf at 16 x 2048 points), 1.5e-8 against 1.8e-1 at 33 x 2047,
                0 in the ten other cases: the products G_i p_hi, G_i p_lo are short and the kernel's fp32 sums hold nearly all of them.
The cases (dect_exact.CASES) are the smallest shapes that reach each regime of the launch: one valid lane, idle waves, 2 + 3 tiles on
two workgroups, the reduce's second pass of 32 partial images, the atomic and the gathered route of the plane gradient on both sides
of 256 and 4096 queries per scene, exactly one persistent round, ragged second rounds of the backward and of the forward, the c5
shape, and the giga_aff (head set 7), giga_geo (8) and giga_detach models.
The six rounded-operand cases by model and weight family that this harness added to tests/test_gpu_train16.py
(test_bf16_decoder_against_operand_rounded_reference_by_model; none left out) measure, as worst relative L2 error of a parameter
gradient against the bound of 8e-3: giga he-11 (3, 300) 2.8e-5, giga spread (3, 300) 1.9e-4, giga nobias (1, 64) 7.6e-8,
giga_aff (3, 0) 3.7e-8, giga_geo (0, 300) 4.6e-6, giga_detach (1, 256) 1.1e-5 (few points: hardly any tipped rounding)."""
import os
import sys

import pytest
import torch

from giga_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_exact as X  # noqa: E402

pytestmark = pytest.mark.gpu


def _same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("fam", X.FAMILIES)
@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_bf16_decoder_is_exact_on_exact_data(case, fam):
    hp, detach, B, N, M = case
    d = X.data(case, fam)
    ref = X.reference(case, fam)
    assert not any(v["stat"]["changed"] for v in ref.heads.values())
    x = torch.from_numpy(synth.tsdf_batch(500, B))
    runs = [X.run_bf16_decoder(X.state_dict(fam), hp, detach, x, d["pos"], d["pos_occ"], d["douts"], planes=d["planes"])
            for _ in range(2)]
    got = runs[0]
    assert torch.equal(got["planes"], d["planes"])           # the decoders did sample the test's planes
    for k, bound in ref.bounds.items():
        err = (got[k].double() - ref.values[k].double()).abs()
        print(f"{X.case_id(case)} {fam} {k}: worst error {float(err.max()):.3e}, bound there "
              f"{float(bound.flatten()[err.argmax()]):.3e}, worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert X.mismatches(got, ref) == []
    assert sorted(k for k in got if k.startswith("grad/")) == sorted(k for k in ref.values if k.startswith("grad/"))
    for k in got:
        assert _same_bytes(got[k], runs[1][k]), ("second run differs", k)
