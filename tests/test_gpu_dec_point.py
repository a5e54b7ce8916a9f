"""GPU tests of decoder_f32_point_kernel (csrc/giga_decoder.hip): the exact-fp32 decoder for ONE query per scene, one workgroup per
(point, head), GEMVs on the VALU over the packed fp32 fragments.  Held to the float64 reference (tests/ref64.py) on planes from a
real encoder call, to the tile kernel it replaces (GIGA_DEC32_POINT=0, same process), to exact arithmetic on small-integer data,
and to itself run twice; the launch probe names the kernel that actually ran, so the dispatch bound is checked too."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

from giga_amd import _capi, networks, synth, weights
from giga_amd.convonet import _planes_to_nhwc, decode_heads, decoder_plan
from oracle import giga_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ref64  # noqa: E402
import test_gpu_f16_exact as f16_exact  # noqa: E402  (its integer state dict)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HEADS = ref64.HEADS
def _point_bound():
    """DEC32_POINT_MAX_P of csrc/giga_dec_plan.h (set from profiles/dec_point/sweep.txt), asked of the library's plan: the largest
    one-query launch that gets the point kernel when no knob is set (a bound can be at most the tile rule's 3072)."""
    saved = {k: os.environ.pop(k) for k in ("GIGA_DEC32_POINT", "GIGA_DEC32_TILE") if k in os.environ}
    try:
        return max(P for P in range(1, 3073) if decoder_plan(P, 1, 0, 1, 0)["kernel"] == "decoder_f32_point_kernel")
    finally:
        os.environ.update(saved)


POINT_MAX_P = _point_bound()
ATOL = 1e-5                  # the bound tests/test_gpu_point_grad.py uses for N == 1 between the fp32 kernels
MASKS = (7, 8, 2)            # the three grasp heads, occupancy, a single head (rot: the four-wide output)
_CACHE = {}


@contextlib.contextmanager
def knob(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


def _setup(seed, B):
    """(net, sd, nhwc planes on the device, the same planes as the reference's dict on the CPU), computed once per (seed, B)."""
    if ("net", seed) not in _CACHE:
        net = networks.get_network("giga")
        net.load_state_dict(weights.make_state_dict(seed))
        _CACHE["net", seed] = net.to(DEV).eval().set_precision("fp32")
    net = _CACHE["net", seed]
    if (seed, B) not in _CACHE:
        x = torch.from_numpy(synth.tsdf_batch(seed, B))
        with torch.no_grad():
            c = net.encode_inputs(x.to(DEV))
        torch.cuda.synchronize()
        _CACHE[seed, B] = (c, {k: c[k].cpu() for k in O.PLANES})
    c, planes = _CACHE[seed, B]
    return net, {k: v.detach().cpu() for k, v in net.state_dict().items()}, c, planes


def _pix32(p):
    """The kernels' pixel coordinate of a coordinate p, operation by operation in fp32 (csrc/giga_dev.h norm_coord, pix_coord)."""
    f = np.float32
    v = f(f(p) / f(1.00001)) + f(0.5)
    v = f(0.99999) if v >= f(1.0) else f(0.0) if v < f(0.0) else f(v)
    g = f(f(2.0) * v - f(1.0))
    return float(min(max(f(f(f(g + f(1.0)) * f(0.5)) * f(39.0)), f(0.0)), f(39.0)))


def _boundary_coords():
    """{k: p} with _pix32(p) == k EXACTLY: fp32 neighbours of (k / 39 - 0.5) * 1.00001 are searched, since that value itself lands
    within an ulp of k on either side.  Not every k has such a p (the normalised coordinate's grid is coarser than half an ulp
    of some k; pixel 39 is out of reach, the normalisation clamps at 0.99999); pixel 0 is the lower clamp."""
    tab = {}
    for k in range(40):
        lo = hi = np.float32((k / 39.0 - 0.5) * 1.00001)
        cands = [lo]
        for _ in range(64):
            lo, hi = np.nextafter(lo, np.float32(-1)), np.nextafter(hi, np.float32(1))
            cands += [lo, hi]
        for c in cands:
            if _pix32(c) == float(k):
                tab[k] = c
                break
    return tab


BOUNDARY = _boundary_coords()


def _points(first, B, shift):
    """(B, 1, 3): scene b is of kind (b + shift) % 3 -- 0 interior, 1 exactly on cell boundaries of its planes (all three pixel
    coordinates whole numbers in the kernels' own fp32 arithmetic, BOUNDARY; pixel 0 among them), 2 outside [-0.5, 0.5] (the
    clamped gather of golden G2b)."""
    assert 0 in BOUNDARY and len(BOUNDARY) >= 20, sorted(BOUNDARY)
    ks = np.array(sorted(BOUNDARY))
    p = synth.query_points(first, B, 1, stream=3, half_width=0.5).copy()
    out = synth.query_points(first, B, 1, stream=4, half_width=0.9)
    rng = np.random.default_rng([5, first])
    for b in range(B):
        kind = (b + shift) % 3
        if kind == 1:
            k = ks[rng.integers(0, len(ks), 3)]
            if b % 2 == 0:
                k[b // 2 % 3] = 0
            p[b, 0] = [BOUNDARY[int(i)] for i in k]
            assert all(_pix32(v) == float(i) for v, i in zip(p[b, 0], k))
        elif kind == 2:
            o = out[b, 0]
            o[np.argmax(np.abs(o))] = np.float32(0.7 if b % 4 < 2 else -0.7)          # at least one coordinate is outside
            p[b, 0] = o
    return torch.from_numpy(p)


def _run(c, p, blob, mask, post=True):
    """(outputs, kernel expression of the launch): one decode_heads call bracketed by the library's launch probe."""
    L = _capi.lib()
    ev = _CACHE.setdefault("ev", (L.giga_event_create(), L.giga_event_create()))
    L.giga_launch_probe(L.giga_launch_count() + 1, ev[0], ev[1])
    try:
        with torch.no_grad():
            out = decode_heads(c.nhwc, p, blob, mask, "fp32", post)
        torch.cuda.synchronize()
        name = (L.giga_launch_probe_name() or b"").decode()
    finally:
        L.giga_launch_probe(0, None, None)
    return out, name


CASES = [(seed, B, shift) for seed in (7, 11) for B, shift in ((1, 0), (1, 1), (1, 2), (3, 0), (32, 0))]


@pytest.mark.parametrize("seed, B, shift", CASES)
def test_point_kernel_matches_float64_and_tile_kernel(seed, B, shift):
    net, sd, c, planes = _setup(seed, B)
    blob = net.packed_blob(DEV)
    p = _points(seed + B, B, shift)
    _, ref = ref64.heads(sd, planes, p)
    for mask in MASKS:
        got, name = _run(c, p.to(DEV), blob, mask)
        assert "decoder_f32_point_kernel" in name, name
        with knob("GIGA_DEC32_POINT", "0"):
            tile, tname = _run(c, p.to(DEV), blob, mask)
        assert "decoder_f32_tile_kernel" in tname, tname
        again, _ = _run(c, p.to(DEV), blob, mask)
        assert set(got) == {h for i, h in enumerate(HEADS) if mask >> i & 1}
        for h, g in got.items():
            r = ref[h].reshape(g.shape)
            e64 = float((g.cpu().double() - r).abs().max())
            et = float((g - tile[h]).abs().max())
            print(f"seed {seed} B {B} shift {shift} mask {mask} {h}: vs float64 {e64:.3e}  vs tile kernel {et:.3e}")
            assert e64 <= ATOL, (mask, h, e64)
            assert et <= ATOL, (mask, h, et)
            assert torch.equal(g, again[h]), (mask, h)         # no atomics: two runs of the same call are bit-identical


def test_dispatch_bound_and_fallback():
    """P == bound runs the point kernel, P == bound + 1 does not (the tile kernel's own rule applies: one head, 9 tiles <= 96).
    GIGA_DEC32_TILE=0 ALONE means the general kernel on both sides of the bound, GIGA_DEC32_POINT=0 alone the tile kernel, a
    value above 1 moves the bound.  All of them agree with float64."""
    seed, B = 7, POINT_MAX_P + 1
    net, sd, c, planes = _setup(seed, B)
    blob = net.packed_blob(DEV)
    p = _points(3, B, 0)
    _, ref = ref64.heads(sd, planes, p, names=("decoder_tsdf", "decoder_rot"))

    class Sub:                                                  # the first POINT_MAX_P scenes
        nhwc = c.nhwc[:, :POINT_MAX_P].contiguous()

    psub = p[:POINT_MAX_P].to(DEV)
    for mask, h in ((8, "decoder_tsdf"), (2, "decoder_rot")):
        runs = {"at": _run(Sub, psub, blob, mask), "above": _run(c, p.to(DEV), blob, mask)}
        with knob("GIGA_DEC32_TILE", "0"):
            runs["TILE=0 above"] = _run(c, p.to(DEV), blob, mask)
            runs["TILE=0 at"] = _run(Sub, psub, blob, mask)
        with knob("GIGA_DEC32_POINT", "0"):
            runs["POINT=0 at"] = _run(Sub, psub, blob, mask)
        with knob("GIGA_DEC32_POINT", str(POINT_MAX_P + 1)):
            runs["POINT=bound+1 above"] = _run(c, p.to(DEV), blob, mask)
        with knob("GIGA_DEC32_POINT", "-3"):                    # not a bound: the default stays
            runs["POINT=-3 at"] = _run(Sub, psub, blob, mask)
        want = {"at": "decoder_f32_point_kernel", "above": "decoder_f32_tile_kernel", "TILE=0 above": "decoder_f32_kernel",
                "TILE=0 at": "decoder_f32_kernel", "POINT=0 at": "decoder_f32_tile_kernel",
                "POINT=bound+1 above": "decoder_f32_point_kernel", "POINT=-3 at": "decoder_f32_point_kernel"}
        r = ref[h].reshape(runs["above"][0][h].shape)
        for what, (out, name) in runs.items():
            assert want[what] in name, (mask, what, name)
            g = out[h]
            e = float((g.cpu().double() - r[:g.shape[0]]).abs().max())
            print(f"mask {mask} {what}: {want[what]}  vs float64 {e:.3e}")
            assert e <= ATOL, (mask, what, e)


def test_point_kernel_is_exact_on_integer_data():
    """Small-integer planes, weights, biases and points: every product and partial sum of the gather and of the eleven layers is
    exactly representable in fp32, so the result does not depend on the summation order and the kernel must return the exact
    values bit for bit -- this pins the k-slot maps, the fragment order, ReLU, the residual adds and the cross-half add.
    Coordinates are -2, -1 (clamped to pixel 0: tap weights 1, 0, 0, 0) and 0 (pixel 19.5: tap weights 1/2 or 1/4)."""
    sd = f16_exact._integer_state_dict(weights.make_state_dict(7), 11)
    g = torch.Generator().manual_seed(5)
    for h in HEADS:
        sd[f"{h}.fc_p.weight"] = torch.randint(-1, 2, (32, 3), generator=g).float()
    net = networks.get_network("giga")
    net.load_state_dict(sd)
    net = net.to(DEV).eval().set_precision("fp32")
    blob = net.packed_blob(DEV)
    for B in (3, 32):
        planes = {k: torch.randint(-2, 3, (B, 32, 40, 40), generator=g).float() for k in O.PLANES}
        p = torch.randint(-2, 1, (B, 1, 3), generator=g).float()
        raw, _ = ref64.heads(sd, planes, p)
        class C:
            nhwc = _planes_to_nhwc({k: v.to(DEV) for k, v in planes.items()}, "fp32")

        out = {}
        for mask in (7, 8):                                     # raw outputs: no sigmoid, no normalisation
            o, name = _run(C, p.to(DEV), blob, mask, post=False)
            assert "decoder_f32_point_kernel" in name, name
            out.update(o)
        for h in HEADS:
            want = raw[h].reshape(out[h].shape)
            assert float((want * 4 - (want * 4).round()).abs().max()) == 0 and float(want.abs().max()) < 2 ** 20, h
            assert float(want.abs().max()) > 0, h
            assert torch.equal(out[h].cpu().double(), want), (B, h, float((out[h].cpu().double() - want).abs().max()))
