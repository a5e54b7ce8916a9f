"""CPU checks of the float64 reference and families of tests/ref64.py: it agrees with the fp32 oracle and with goldens G1-G3,
the f16x3 split has the operand window include/giga_hip.h states, and the range-relative tolerance of the GPU envelope tests
rejects a realistic kernel bug (one U-Net layer with plain f16 operands) by a wide margin."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import synth, weights
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402

GOLDEN_TOL = 2e-5        # tests/test_oracle_goldens.py


def _close(a, b, tol):
    err = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()
    assert err <= tol, f"max abs err {err:.3e} > {tol}"


def test_encoder_matches_oracle_and_g1(golden, sd7):
    g = golden("g1_encoder.npz")
    x = torch.from_numpy(synth.tsdf_batch(0, 2))
    pl = ref64.encoder(sd7, x)
    ref = O.encoder_forward(sd7, x)
    for k in O.PLANES:
        assert pl[k].dtype == torch.float64
        _close(pl[k], ref[k], GOLDEN_TOL)
        _close(pl[k][:, :, ::2, ::2], g[f"plane_{k}_s2"], GOLDEN_TOL)
        _close(pl[k][0, 5], g[f"plane_{k}_b0c5"], GOLDEN_TOL)
        s = g[f"plane_{k}_sums"]
        assert abs(pl[k].sum().item() - s[0]) <= 1e-5 * max(1.0, s[1])


def test_heads_match_oracle_and_g2(golden, sd7):
    g = golden("g2_decoder.npz")
    x = torch.from_numpy(synth.tsdf_batch(0, 2))
    p = torch.from_numpy(synth.query_points(0, 2, 2048, stream=1, half_width=0.6))
    planes = ref64.encoder(sd7, x)
    raw, out = ref64.heads(sd7, planes, p)
    for h, name in zip(ref64.HEADS, ("qual", "rot", "width", "tsdf")):
        _close(raw[h], g["raw_" + h], GOLDEN_TOL)
        _close(out[h], g[name], GOLDEN_TOL)
    q, r, w, t = O.model_forward(sd7, x, p, p_tsdf=p)
    for got, want in ((out["decoder_qual"], q), (out["decoder_rot"], r), (out["decoder_width"], w), (out["decoder_tsdf"], t)):
        _close(got, want, GOLDEN_TOL)


def test_lattice_matches_g3(golden, sd7):
    g = golden("g3_lattice.npz")
    lat = torch.from_numpy(synth.inference_lattice())
    planes = ref64.encoder(sd7, torch.from_numpy(synth.tsdf_batch(int(g["scene"]), 1)))
    _, out = ref64.heads(sd7, planes, lat, ref64.HEADS[:3])
    sub = g["subset"]
    for h, name in zip(ref64.HEADS[:3], ("qual", "rot", "width")):
        _close(out[h][0, sub], g[name], GOLDEN_TOL)
        s = g[name + "_sums"]
        assert abs(out[h].sum().item() - s[0]) <= 2e-5 * max(1.0, s[1])


def test_fp32_oracle_is_within_a_tenth_of_the_tolerance_of_float64(sd7):
    """The fp32 oracle's own distance from float64 (seed 7, scenes 0-1: ~5e-7 of range) is small next to ref64.TOL, so
    holding the kernels to float64 is not holding them to the oracle's rounding."""
    x = torch.from_numpy(synth.tsdf_batch(0, 2))
    r64, r32 = ref64.encoder(sd7, x), O.encoder_forward(sd7, x)
    worst = max(ref64.planes_err(r32, r64, k) for k in range(2))
    assert worst < 0.1 * min(ref64.TOL.values()), worst


def _one_layer_f16(layer):
    """unet_forward's `rnd` hook rounding the input and weight of ONE convolution (layer-th of the 13, in unet_stages order)
    to f16: the 'lo products dropped' mutation of the f16x3 arithmetic on that layer."""
    calls = [0]

    def rnd(t):
        i = calls[0]
        calls[0] += 1
        return t.half().float() if (i % 26) // 2 == layer else t
    return rnd


@pytest.mark.parametrize("layer", range(13))
def test_tolerance_rejects_one_layer_in_f16(sd7, layer):
    """Sensitivity check: the comparison the GPU envelope tests apply (range-relative error against float64) rejects the
    oracle with one layer's operands in plain f16 by at least 4x the tolerance, for every layer."""
    x = torch.from_numpy(synth.tsdf_batch(0, 2))
    r64 = ref64.encoder(sd7, x)
    with torch.no_grad():
        mutated = O.encoder_forward(sd7, x, rnd=_one_layer_f16(layer))
    err = max(ref64.planes_err(mutated, r64, k) for k in range(2))
    assert err >= 4 * max(ref64.TOL.values()), err


def test_range_err_flags_non_finite_output():
    ref = torch.linspace(-1, 1, 10, dtype=torch.float64)
    got = ref.clone()
    assert ref64.range_err(got, ref) == 0
    got[3] = float("nan")
    assert ref64.range_err(got, ref) == float("inf")


def _split_worst(lo_exp, hi_exp, n=20000, seed=0):
    """Worst relative error of hi + lo over values log-uniform in [2^lo_exp, 2^hi_exp), both signs."""
    rng = np.random.default_rng(seed)
    v = (np.exp2(rng.uniform(lo_exp, hi_exp, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    hi, lo = ref64.f16x3_split(v)
    return float(np.max(np.abs((hi.astype(np.float64) + lo) - v) / np.abs(v.astype(np.float64))))


def test_f16x3_split_window():
    """The operand window of precision 2 (include/giga_hip.h): hi + lo carries v to 2^-22 relative
    for 2^-3 <= |v| < 65520; below 2^-3 lo is subnormal and the error is 2^-25 absolute (2^-17 relative at 2^-8, 2^-13 at
    2^-12); from 65520 up hi = f16(v) is infinite."""
    assert _split_worst(-3, 15.99) <= 2.0 ** -22
    assert 2.0 ** -19 < _split_worst(-8, -7) <= 2.0 ** -17
    assert 2.0 ** -15 < _split_worst(-12, -11) <= 2.0 ** -13
    hi, _ = ref64.f16x3_split(np.array([65504.0, 65519.0, 65520.0, -70000.0], np.float32))
    assert np.isfinite(hi[:2]).all() and np.isinf(hi[2:]).all()


def test_families_are_what_they_say():
    he7 = weights.make_state_dict_numpy(7)
    sp = ref64.weight_family_numpy("spread")
    nb = ref64.weight_family_numpy("nobias")
    nf = ref64.weight_family_numpy("nobias-nofcp")
    assert set(sp) == set(he7) == set(nb) == set(nf)
    for k, v in he7.items():
        if k.endswith("bias"):
            assert np.abs(sp[k]).max() <= 0.5 and not nb[k].any() and not nf[k].any()
        else:
            axis = 1 if k.endswith("upconv.weight") else 0
            gain = (sp[k] / np.where(v == 0, 1, v)).swapaxes(0, axis).reshape(v.shape[axis], -1)[:, 0]
            assert (gain >= 0.25 - 1e-6).all() and (gain <= 4 + 1e-6).all(), k
            np.testing.assert_array_equal(nb[k], v)
            assert (not nf[k].any()) if ".fc_p." in k else np.array_equal(nf[k], v)
    for fam in ref64.INPUT_FAMILIES:
        x = ref64.input_family(fam, 6)
        assert x.shape == (6, 40, 40, 40) and x.dtype == np.float32 and x.min() >= 0 and x.max() <= 1
        assert len({xi.tobytes() for xi in x}) == 6, fam
    st = ref64.input_family("structured", 3)
    assert ((st == 0).mean() > 0.3) and ((st > 0) & (st < 1)).any()
