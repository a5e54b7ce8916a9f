"""GPU tests of the MFMA chain of decoder_f32_kernel<T, LATTICE> (csrc/giga_decoder.hip): per layer and tile one run of 16 ReLUs
and one uninterrupted run of 16 MFMAs, accumulators in VGPRs, the bias rows as the C operand of a layer's first MFMA, no zero-weight
aux MFMA behind block 0.  Every head output is held to the float64 reference (tests/ref64.py) on planes from a real encoder call
and to itself run twice; the launch probe names the kernel that ran and its T.

The shapes are the smallest at which the body takes another path: one tile per wave with a ragged second tile; four heads, one
workgroup each (the dispatch spreads heads over workgroups while they fit the chip) and rot's four-wide store; several scenes
with a tile straddling two of them; four heads in ONE workgroup, which reloads the weight image per head (260 tiles: 65 point
batches x 4 heads no longer fit 256 workgroups); both sides of the two-tiles-per-wave threshold of 2048 tiles, ragged and exact,
and two heads at two tiles per wave; the lattice instantiation at R = 8."""
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, convonet, synth
from giga_amd.convonet import decode_heads

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402
import test_gpu_dec_point as dec_point  # noqa: E402  (its encoder set-up and its table of exact cell-boundary coordinates)
from lattice_lins import grid_points, lin_family  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = ref64.HEADS
ATOL = dec_point.ATOL        # 1e-5: the bound tests/test_gpu_dec_point.py holds the fp32 kernels to


def _points(first, B, N):
    """(B, N, 3): point i of scene b is of kind (i + b) % 3 -- 0 interior, 1 exactly on cell boundaries of its planes (all three
    pixel coordinates whole numbers in the kernels' own fp32 arithmetic, pixel 0 among them), 2 outside [-0.5, 0.5]."""
    tab = dec_point.BOUNDARY
    assert 0 in tab and len(tab) >= 20, sorted(tab)
    vals = np.array([tab[k] for k in sorted(tab)], np.float32)
    p = synth.query_points(first, B, N, stream=3, half_width=0.5).copy()
    out = synth.query_points(first, B, N, stream=4, half_width=0.9)
    rng = np.random.default_rng([6, first])
    kind = (np.arange(N)[None, :] + np.arange(B)[:, None]) % 3
    on = vals[rng.integers(0, len(vals), (B, N, 3))]
    on[:, ::2, 0] = tab[0]                                      # pixel 0: the lower clamp
    far = out.copy()
    ax = np.abs(far).argmax(-1)
    sign = np.where(rng.integers(0, 2, (B, N)) > 0, 0.7, -0.7).astype(np.float32)
    np.put_along_axis(far, ax[..., None], sign[..., None], -1)  # at least one coordinate is outside
    p[kind == 1] = on[kind == 1]
    p[kind == 2] = far[kind == 2]
    assert (np.abs(p[kind == 2]).max(-1) > 0.5).all() and (np.abs(p[kind == 0]) <= 0.5).all()
    return torch.from_numpy(p)


def _run(nhwc, p, blob, mask, nth=1):
    """(outputs, name of the nth kernel launched by one decode_heads call), through the library's launch probe."""
    L = _capi.lib()
    ev = dec_point._CACHE.setdefault("ev", (L.giga_event_create(), L.giga_event_create()))
    L.giga_launch_probe(L.giga_launch_count() + nth, ev[0], ev[1])
    try:
        with torch.no_grad():
            out = decode_heads(nhwc, p, blob, mask, "fp32", True)
        torch.cuda.synchronize()
        name = (L.giga_launch_probe_name() or b"").decode()
    finally:
        L.giga_launch_probe(0, None, None)
    return out, name


def _is_chain_kernel(name, T, lattice):
    """The probe gives the kernel's name as the runtime knows it: demangled or mangled."""
    plain = f"decoder_f32_kernel<{T}, {'true' if lattice else 'false'}>"
    mangled = f"decoder_f32_kernelILi{T}ELb{int(lattice)}EE"
    return plain in name.replace("(int)", "").replace("(bool)", "") or mangled in name


def _check(tag, got, again, raw, ref, B, mask):
    assert set(got) == {h for i, h in enumerate(HEADS) if mask >> i & 1}
    for h, g in got.items():
        assert torch.equal(g, again[h]), (tag, h)               # no atomics: two runs of the same call are bit-identical
        worst, r, z = 0.0, ref[h].reshape(g.shape), raw[h].reshape(g.shape)
        for b in range(B):
            e = ref64.rot_err(g[b], r[b], z[b]) if h == "decoder_rot" else ref64.range_err(g[b], r[b])
            worst = max(worst, e)
        print(f"{tag} mask {mask} {h}: vs float64 {worst:.3e}")
        assert worst <= ATOL, (tag, mask, h, worst)


#        B, N,     mask, T
CASES = [(1, 33,    8,   1),      # two tiles, the second ragged
         (1, 40,    15,  1),      # four heads, rot's four-wide store
         (3, 700,   7,   1),      # several point batches per workgroup, a tile straddling scenes
         (1, 8300,  15,  1),      # 260 tiles: all four heads in one workgroup, the image reloaded per head
         (1, 65505, 8,   2),      # 2048 tiles, the last ragged: two tiles per wave
         (2, 32768, 8,   2),      # 2048 tiles exactly
         (1, 65504, 8,   1),      # 2047 tiles: the last launch with one tile per wave
         (2, 32768, 6,   2)]      # two tiles per wave and two heads: the image reloaded with both tiles' features held


@pytest.mark.parametrize("seed", (7, 11))
@pytest.mark.parametrize("B, N, mask, T", CASES)
def test_chain_matches_float64(seed, B, N, mask, T):
    net, sd, c, planes = dec_point._setup(seed, B)
    blob = net.packed_blob(DEV)
    p = _points(seed + N, B, N)
    names = tuple(h for i, h in enumerate(HEADS) if mask >> i & 1)
    raw, ref = ref64.heads(sd, planes, p, names)
    got, name = _run(c.nhwc, p.to(DEV), blob, mask)
    assert _is_chain_kernel(name, T, False), name
    again, _ = _run(c.nhwc, p.to(DEV), blob, mask)
    _check(f"seed {seed} B {B} N {N} T {T}", got, again, raw, ref, B, mask)


@pytest.mark.parametrize("seed", (7, 11))
def test_lattice_chain_matches_float64(seed):
    """giga_decoder_forward_lattice at R = 8, fp32, the three grasp heads: the resample kernel, then decoder_f32_kernel<1, true>.
    The mesh recipe's lattice has both ends outside the cube."""
    B, R, mask = 3, 8, 7
    net, sd, c, planes = dec_point._setup(seed, B)
    blob = net.packed_blob(DEV)
    lin = lin_family("b", R)
    pos = convonet.register_lattice(grid_points(lin).to(DEV), lin)
    raw, ref = ref64.heads(sd, planes, grid_points(lin).expand(B, -1, -1), HEADS[:3])
    fast = convonet.LATTICE_STATS["fast"]
    got, first = _run(c.nhwc, pos, blob, mask, nth=1)
    again, second = _run(c.nhwc, pos, blob, mask, nth=2)
    assert convonet.LATTICE_STATS["fast"] == fast + 2
    assert "lattice_resample" in first and _is_chain_kernel(second, 1, True), (first, second)
    _check(f"seed {seed} lattice R {R} B {B}", got, again, raw, ref, B, mask)
