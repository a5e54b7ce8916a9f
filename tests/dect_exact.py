"""Data on which the training decoders -- bf16 (csrc/giga_decoder_train16.hip) and fp32 (csrc/giga_decoder_bwd.hip) -- are EXACT,
their reference, and a harness that puts test-chosen planes in front of the decoder kernels (test helper;
tests/test_dect_exact_host.py pins the data on the CPU, tests/test_gpu_train16_shapes.py and tests/test_gpu_dec32_shapes.py hold
the kernels to it).

Two valid bf16 evaluations of real-valued data decorrelate (tests/test_gpu_train16.py), so a comparison on such data is statistical.
Here every operand that tests/dect_ref.py rounds to bf16 already is a bf16 value and every sum fits fp32 exactly: integer planes in
{-2..2}, hidden matrices with two +-1 entries per row (eight in fc_out), integer biases, fc_p.weight in {-1, 0, 1}, integer upstream
gradients for `width` and the occupancy logits and zero ones for `qual` and `rot` (sigmoid and normalize are not exact).  The result
then does not depend on the summation order, on the atomics or on which wave summed which tile: the GPU returns the reference bit for bit.
  family A  every coordinate in {-2, -1, 0}: -2 and -1 clamp to pixel 0, 0 is pixel 19.5: tap weights 1, 1/2, 1/4, many points per cell.
  family B  coordinates that are whole pixels 0..38 in the kernels' own fp32 arithmetic (BOUNDARY of tests/test_gpu_dec_point.py), drawn
            per axis: the scatter spreads over the planes.  They are no bf16 values, so fc_p.weight = 0 (forward and every other
            gradient stay exact) and the gradient of fc_p.weight alone is held to the worst case of an fp32 sum (fcp_bound).
Features are sampled at the pixel coordinate the kernels compute (csrc/giga_dev.h norm_coord, pix_coord, bilin_setup: fp32), summed in
float64: float64 pixel coordinates (tests/ref64.py) miss a whole pixel of family B by 1e-7 and would put that much on a second tap.
  family C  (fp32 only) like B, but every coordinate one of EIGHT whole pixels (FAMILY_C_PIXELS): 64 cells per plane, each with
            more than 32 of a scene's 4096 points -- more long cell lists than plane_gather_kernel ranks with the whole workgroup.
precision "fp32" is the fp32 training decoder: the same chain with NO rounding (dect_ref.bf is the identity: fp32 holds operands
of 9 and more significant bits that bf16 does not, so the rounding reference would be wrong for it), and the `qual` head has a
gradient too: the harness hands giga_backward outs[0] = 0.5 (sigmoid' = 1/4 exactly) and upstream gradients in {-8, -4, 0, 4, 8},
so that dO = d / 4 is in {-2..2} like `width`'s.  `rot` keeps a zero upstream gradient in both (normalize backward is not exact)."""
import contextlib
import ctypes
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dect_ref as R  # noqa: E402
import test_gpu_dec_point as dec_point  # noqa: E402  (BOUNDARY)
import test_gpu_f16_exact as f16_exact  # noqa: E402  (its integer state dict)
from giga_amd import weights  # noqa: E402
from oracle import giga_oracle as O  # noqa: E402

HEADS = weights.HEADS
HEAD_BITS = {"decoder_qual": 1, "decoder_rot": 2, "decoder_width": 4, "decoder_tsdf": 8}
PRECISIONS = ("bf16", "fp32")
# the heads with a nonzero upstream gradient
EXACT_HEADS = {"bf16": ("decoder_width", "decoder_tsdf"), "fp32": ("decoder_qual", "decoder_width", "decoder_tsdf")}
RES, CD = 40, 32

# (head set, detach the occupancy head's plane gradient, B, N grasp queries, M occupancy queries).  tiles = ceil(P / 32); the backward
# runs min(ceil(tiles / 4), 256) workgroups, the forward min(ceil(tiles / 8), 256).
CASES = [
    (15, False, 1, 1, 1),        # one valid lane in the whole launch, both calls
    (15, False, 1, 33, 255),     # 2 tiles: two idle waves; occupancy one below the gather threshold (atomic route)
    (15, False, 3, 43, 256),     # 129 points = 5 tiles on 2 workgroups (2 + 3); first gathered size
    (15, False, 7, 3, 600),      # 4200 points, 132 tiles, 33 workgroups: the reduce's second pass of 32
    (15, False, 2, 1, 4097),     # above PS_MAXN: atomic route with 8194 points, 65 workgroups
    (15, False, 16, 1, 2048),    # 1024 tiles: 256 workgroups, exactly one round
    (15, False, 17, 37, 2047),   # 1088 tiles on 256 workgroups: ragged second round, last tile 15 points; grasp call 629 points
    (15, False, 32, 1, 2048),    # the c5 shape
    (15, False, 33, 1, 2047),    # 2111 tiles: the forward's second round too, last tile 31 points
    (7, False, 5, 2, 0),         # giga_aff: no occupancy head, other parameter offsets
    (8, False, 3, 0, 300),       # giga_geo: occupancy head alone
    (15, True, 4, 1, 256),       # giga_detach: the plane gradient is the grasp heads' only
]
FAMILIES = ("A", "B")
FAMILY_C_PIXELS = (0, 12, 15, 18, 24, 27, 30, 33)
# fp32 only (csrc/giga_decoder_bwd.hip launch_decoder_backward; bwd32_launch below reads its plan)
CASES32_NEW = [
    ((7, False, 32, 340, 0), ("A", "B")),     # 10 880 points, 85 batches: 85 x 3 = 255, the last shape with one workgroup per head
    ((7, False, 32, 341, 0), ("A", "B")),     # 10 912 points, 86 batches: 258 > 256, the first shape where one workgroup walks three heads
    ((8, False, 2, 0, 4096), ("A", "C")),     # the gather at its upper bound: C 64 long cells per plane, A four cells of about 1000 points
    ((8, False, 2, 0, 4097), ("C",)),         # one past PS_MAXN: atomics on the same kind of points
]
CASES32 = [(c, f) for c in CASES for f in FAMILIES] + [(c, f) for c, fams in CASES32_NEW for f in fams]
WEIGHT_SEED = 30                 # (of 40 seeds tried, ten keep every operand a bf16 value and every gradient matrix 10 % dense)
# {(head set, B, N, M[, family]): seed} of the cases that miss the conditions of tests/test_dect_exact_host.py with their default seed
# (family A at 65 536 points: a few activations of 9 significant bits; two or four grasp points: a gradient matrix under 10 % dense)
# (the one-point case: the densest of 3000 seeds per family, see ONE_POINT in tests/test_dect_exact_host.py)
DATA_SEED = {(15, 2, 1, 4097): 93, (15, 4, 1, 256): 2, (15, 32, 1, 2048): 5, (15, 33, 1, 2047): 1,
             (15, 1, 1, 1, "A"): 1610, (15, 1, 1, 1, "B"): 662}


# fp32 only: `qual` has a gradient there, and with one to four grasp points its matrices miss the density with the seeds above
# ((head set, B, N, M, family): the first of seeds 1.. that holds every condition of tests/test_dect_exact_host.py; the one-point
# case: 3 of 6000 seeds reach 1/16 in family A, 2 in B)
DATA_SEED32 = {(15, 2, 1, 4097, "A"): 277, (15, 2, 1, 4097, "B"): 147, (7, 5, 2, 0, "A"): 1, (15, 4, 1, 256, "A"): 36,
               (15, 4, 1, 256, "B"): 8, (15, 1, 1, 1, "A"): 30, (15, 1, 1, 1, "B"): 1109}


def data_seed(case, fam, precision="bf16"):
    hp, _, B, N, M = case
    if precision == "fp32" and (hp, B, N, M, fam) in DATA_SEED32:
        return DATA_SEED32[hp, B, N, M, fam]
    return DATA_SEED.get((hp, B, N, M, fam), DATA_SEED.get((hp, B, N, M), 100 + hp + 16 * B + 1000 * N + 100000 * M))


def case_id(c):
    return f"{c[0]}{'d' if c[1] else ''}-{c[2]}-{c[3]}-{c[4]}"


def case32_id(cf):
    return f"{case_id(cf[0])}-{cf[1]}"


def heads_of(hp):
    return tuple(h for h in HEADS if hp & HEAD_BITS[h])


@functools.lru_cache(maxsize=None)
def state_dict(fam):
    sd = f16_exact._integer_state_dict(weights.make_state_dict(7), WEIGHT_SEED, per_row=2, out_per_row=8, fc_p=True)
    if fam != "A":
        for h in HEADS:
            sd[f"{h}.fc_p.weight"] = torch.zeros(32, 3)
    return sd


@functools.lru_cache(maxsize=2)
def data(case, fam, precision="bf16"):
    """dict: planes (3, B, 40, 40, 32) NHWC fp32, pos (B, N, 3), pos_occ (B, M, 3), douts {head: upstream gradient}.  Where the
    two precisions have the same seed they share everything but `qual`'s upstream gradient (fp32: multiples of 4, drawn from a
    generator of its own)."""
    hp, _, B, N, M = case
    g = torch.Generator().manual_seed(data_seed(case, fam, precision))
    planes = torch.randint(-2, 3, (3, B, RES, RES, CD), generator=g).float()
    if fam == "A":
        draw = lambda n: torch.randint(-2, 1, (B, n, 3), generator=g).float()  # noqa: E731
    else:
        pixels = sorted(dec_point.BOUNDARY) if fam == "B" else FAMILY_C_PIXELS
        vals = torch.tensor([dec_point.BOUNDARY[k] for k in pixels], dtype=torch.float32)
        draw = lambda n: vals[torch.randint(0, len(vals), (B, n, 3), generator=g)]  # noqa: E731
    pos, pos_occ = draw(N), draw(M)

    def upstream(n):
        d = torch.randint(-2, 3, (B, n), generator=g).float()
        if n and d[-1, -1] == 0:                             # the kernel pads idle lanes with the last point of the call
            d[-1, -1] = 1.0
        return d

    douts = {"decoder_qual": torch.zeros(B, N), "decoder_rot": torch.zeros(B, N, 4), "decoder_width": upstream(N),
             "decoder_tsdf": upstream(M)}
    if precision == "fp32":
        g = torch.Generator().manual_seed(data_seed(case, fam, precision) + 1000003)
        douts["decoder_qual"] = 4.0 * upstream(N)
    return dict(planes=planes, pos=pos, pos_occ=pos_occ, douts=douts)


# ---- the features, at the kernels' own pixel coordinates -------------------------------------------------------------------------
def pix_coord(xy):
    """csrc/giga_dev.h pix_coord, operation by operation in fp32."""
    assert xy.dtype == torch.float32
    g = 2.0 * xy - 1.0
    return (((g + 1.0) * 0.5) * 39.0).clamp(0.0, 39.0)


def footprint(p, k):
    """The four taps of the points p (B, N, 3) on plane k as bilin_setup computes them (fp32): [(pixel y * 40 + x (B, N) long,
    weight (B, N) fp32)] in the order o00, o01, o10, o11.  The first index is the cell plane_gather_kernel bins the point by."""
    f = pix_coord(O.normalize_coordinate(p.float(), k))         # (B, N, 2): [..., 0] indexes W, [..., 1] indexes H
    f0 = f.floor()
    a, b = f - f0, (f0 + 1.0) - f
    x0, y0 = f0[..., 0].long(), f0[..., 1].long()
    x1, y1 = (x0 + 1).clamp(max=RES - 1), (y0 + 1).clamp(max=RES - 1)
    return [(y0 * RES + x0, b[..., 0] * b[..., 1]), (y0 * RES + x1, a[..., 0] * b[..., 1]),
            (y1 * RES + x0, b[..., 0] * a[..., 1]), (y1 * RES + x1, a[..., 0] * a[..., 1])]


def sample_features(p, planes):
    """(B, N, 96) float64 of planes {'xz','xy','yz'}: (B, 32, 40, 40), differentiable w.r.t. the planes.  Coordinates, the four
    taps and their weights as bilin_setup computes them (fp32); products and sums in float64."""
    B, N = p.shape[0], p.shape[1]
    cols = []
    for k in O.PLANES:
        img = planes[k].double().permute(0, 2, 3, 1).reshape(B, RES * RES, CD)
        c = 0.0
        for at, w in footprint(p, k):
            tap = torch.gather(img, 1, at[..., None].expand(B, N, CD))
            c = c + tap * w.double()[..., None]
        cols.append(c)
    return torch.cat(cols, dim=-1)


def scatter_planes(p, dc, keep=None, absolute=False):
    """sample_features backward written out: the plane gradients (3, B, 40, 40, 32) float64 of the rows dc (B * N, 96) at the points
    p (B, N, 3), every product and sum in float64.  keep (B * N,) bool: only these points; absolute: of |dc| (the sum that
    dominates every partial sum of the scatter, whatever its order)."""
    B, N = p.shape[0], p.shape[1]
    dc = dc.reshape(B, N, 96).double()
    if absolute:
        dc = dc.abs()
    if keep is not None:
        dc = dc * keep.reshape(B, N, 1).to(dc.dtype)
    out = torch.zeros(3, B, RES * RES, CD, dtype=torch.float64)
    for i, k in enumerate(O.PLANES):
        for at, w in footprint(p, k):
            out[i].scatter_add_(1, at[..., None].expand(B, N, CD), dc[..., CD * i:CD * (i + 1)] * w.double()[..., None])
    return out.view(3, B, RES, RES, CD)


def cells(p):
    """(3, B, N) long: the cell (o00 of bilin_setup) of every point on every plane."""
    return torch.stack([footprint(p, k)[0][0] for k in O.PLANES])


# ---- the fp32 backward's launch arithmetic, read from the library's plan --------------------------------------------------------
def xcd_swizzle(i, n):
    """csrc/giga_dev.h xcd_swizzle, restated (kernel arithmetic, not launch policy: no plan holds it)."""
    m = n & ~7
    return (i & 7) * (m >> 3) + (i >> 3) if i < m else i


def _bwd32_dict(call):
    """The fields of one fp32 call of convonet.decoder_backward_plan under the names the tests use; round2 and last_block follow
    from them: the batches of decoder_bwd_kernel's later persistent rounds (bseq >= grid, through xcd_swizzle) and the points of
    linear_wgrad_kernel's last block."""
    P, nbatch, grid, ksplit, ppb = call["P"], call["nbatch"], call["grid_x"], call["ksplit"], call["pts_per_block"]
    return dict(P=P, nheads=call["nheads"], tiles=call["tiles"], nbatch=nbatch, grid=grid, split=call["heads_per_wg"] == 1,
                round2=sorted(xcd_swizzle(i, nbatch) for i in range(grid, nbatch)),
                nb_total=call["nb_total"], ksplit_cap=call["ksplit_cap"], pts_per_block=ppb, ksplit=ksplit,
                last_block=P - (ksplit - 1) * ppb, gather=call["gather"])


def bwd32_launch(P, nheads, N=0):
    """What launch_decoder_backward (csrc/giga_decoder_bwd.hip) launches for P points and nheads heads in one call, as the
    library's plan says (csrc/giga_dec_bwd_plan.h dec_bwd_call_plan, through convonet.decoder_backward_plan: host only, the built
    library and no device): tiles, nbatch, grid, split (one workgroup per head), nb_total, ksplit_cap, pts_per_block, ksplit.
    N > 0: the call is the occupancy call of P / N scenes, which may write the planes -- gather is the plan's rule for it (the
    caller, giga_backward, also asks that the head is not detached: bwd32_calls); else a grasp call, which never gathers."""
    from giga_amd import convonet
    if N:
        assert nheads == 1 and P % N == 0
        return _bwd32_dict(convonet.decoder_backward_plan(P // N, 0, N, 8)["occ"])
    return _bwd32_dict(convonet.decoder_backward_plan(1, P, 0, (1 << nheads) - 1)["grasp"])


def bwd32_calls(case):
    """{'occ' / 'grasp': the fp32 calls giga_backward (csrc/giga_capi.hip) makes for a case, from its plan}."""
    from giga_amd import _capi, convonet
    hp, detach, B, N, M = case
    plan = convonet.decoder_backward_plan(B, N, M, hp | (_capi.DETACH_OCC if detach else 0))
    return {name: _bwd32_dict(plan[name]) for name in ("occ", "grasp") if plan[name]["runs"]}


# ---- reference -----------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def counting_bf(skip=lambda t: False, identity=False):
    """Wraps dect_ref.bf: stat["changed"] counts the operands a rounding to bf16 changes, stat["max"] is the largest operand.
    identity: the operands are counted but NOT rounded -- the chain of tests/dect_ref.py in fp32 operands."""
    stat = {"changed": 0, "max": 0.0, "calls": 0}
    orig = R.bf

    def bf(t):
        r = orig(t)
        if not skip(t):
            stat["changed"] += int((r != t).sum())
            stat["max"] = max(stat["max"], float(t.abs().max()) if t.numel() else 0.0)
            stat["calls"] += 1
        return t if identity else r

    R.bf = bf
    try:
        yield stat
    finally:
        R.bf = orig


def slice_saved(saved, idx):
    return {k: ([t[idx] for t in v] if isinstance(v, list) else v[idx]) for k, v in saved.items() if k != "dn0"}


def fcp_bound(saved):
    """Worst case of an fp32 sum of the P terms G_i p_i of fc_p.weight's gradient, per element (32, 3): 2 P 2^-23 max_i |G_i p_i|."""
    G = saved["dn0"].double()
    p = saved["p_hi"].double() + saved["p_lo"].double()
    P = G.shape[0]
    return 2.0 * P * 2.0 ** -23 * (G.abs()[:, :, None] * p.abs()[:, None, :]).amax(0)


class Reference:
    """Everything the GPU is compared with, and what the sensitivity check needs to build a defect."""

    def __init__(self, case, fam, precision="bf16", data_of=None):
        """data_of: the precision whose data the reference is evaluated on (default: its own; `qual`'s upstream gradient counts
        only in "fp32")."""
        hp, detach, B, N, M = case
        assert precision in PRECISIONS and (data_of or precision) in PRECISIONS
        d = data(case, fam, data_of or precision)
        sd = state_dict(fam)
        exact = EXACT_HEADS[precision]
        self.case, self.fam, self.sd, self.precision, self.exact_heads = case, fam, sd, precision, exact
        planes = {k: d["planes"][i].permute(0, 3, 1, 2).double().requires_grad_(True) for i, k in enumerate(O.PLANES)}
        self.values, self.bounds, self.heads = {}, {}, {}
        occ_planes = None
        for head in heads_of(hp):
            p = d["pos_occ"] if head == "decoder_tsdf" else d["pos"]
            n = p.shape[1]
            if n == 0:
                for k, shp in weights.giga_param_shapes(heads=[head]).items():
                    if k.startswith(head):
                        self.values["grad/" + k] = torch.zeros(shp)
                continue
            P = B * n
            skip = (lambda t, P=P: t.dim() == 2 and t.shape == (P, 3)) if fam != "A" else (lambda t: False)
            c = sample_features(p, planes)
            with counting_bf(skip, identity=precision == "fp32") as stat:
                raw, saved = R.head_forward(sd, head + ".", c.detach().reshape(P, 96).float(), p.reshape(P, 3))
                dO = d["douts"][head].reshape(P, -1) if head in exact else torch.zeros(P, raw.shape[-1])
                if head == "decoder_qual":                   # (fp32: sigmoid' at the q = 0.5 the harness passes; bf16: zero)
                    dO = dO / 4.0
                g, dc = R.head_backward(sd, head + ".", saved, dO)
            raw = raw.reshape(B, n, -1)
            self.values["raw/" + head] = raw if head == "decoder_rot" else raw[..., 0]
            if head in ("decoder_width", "decoder_tsdf"):    # (the training call returns them raw)
                self.values["out/" + head] = raw[..., 0]
            for k, v in g.items():
                self.values[f"grad/{head}.{k}"] = v.reshape(sd[f"{head}.{k}"].shape)
            if fam != "A" and head in exact:
                self.bounds[f"grad/{head}.fc_p.weight"] = fcp_bound(saved)
            if not (detach and head == "decoder_tsdf"):
                c.backward(dc.reshape(B, n, 96).double())
            else:                                            # kept aside for the sensitivity check, not part of the result
                gp = torch.autograd.grad(c, list(planes.values()), dc.reshape(B, n, 96).double())
                occ_planes = torch.stack([t.permute(0, 2, 3, 1) for t in gp]).float()
            self.heads[head] = dict(saved=saved, dO=dO, stat=stat, P=P, dc=dc, p=p)
        self.values["gplanes"] = torch.stack([(planes[k].grad if planes[k].grad is not None else torch.zeros_like(planes[k]))
                                              .permute(0, 2, 3, 1) for k in O.PLANES]).float()
        self.occ_planes = occ_planes

    def head_grads(self, head, idx=None, relu_mask=None):
        """Parameter gradients of `head` from the points idx (default: all), named like self.values."""
        h = self.heads[head]
        saved, dO = (h["saved"], h["dO"]) if idx is None else (slice_saved(h["saved"], idx), h["dO"][idx])
        with counting_bf(identity=self.precision == "fp32"):
            g, _ = R.head_backward(self.sd, head + ".", dict(saved), dO, relu_mask=relu_mask)
        return {f"grad/{head}.{k}": v.reshape(self.sd[f"{head}.{k}"].shape) for k, v in g.items()}

    def pairs(self, head):
        """{parameter name: (dY, X)} of `head`: the operands of every weight gradient dY^T X (X None: a bias, dY's column sum)."""
        h, pairs = self.heads[head], {}
        with counting_bf(identity=self.precision == "fp32"):
            R.head_backward(self.sd, head + ".", dict(h["saved"]), h["dO"], pairs=pairs)
        return pairs

    def plane_grad(self, head, keep=None, absolute=False):
        """`head`'s share of the plane gradient (3, B, 40, 40, 32) float64, from its dc rows (scatter_planes)."""
        h = self.heads[head]
        return scatter_planes(h["p"], h["dc"], keep=keep, absolute=absolute)


@functools.lru_cache(maxsize=2)
def reference(case, fam, precision="bf16"):
    return Reference(case, fam, precision)


def occ_plane_grad64(sd, planes, pos_occ, dout):
    """(3, B, 40, 40, 32) float64: the occupancy head's plane gradient on ANY data -- planes (3, B, 40, 40, 32), queries (B, M, 3),
    upstream gradient (B, M) -- as the float64 sum (scatter_planes) of the dc rows of the unrounded chain of tests/dect_ref.py."""
    B, M = pos_occ.shape[0], pos_occ.shape[1]
    c = sample_features(pos_occ, {k: planes[i].permute(0, 3, 1, 2).double() for i, k in enumerate(O.PLANES)})
    with counting_bf(identity=True):
        _, saved = R.head_forward(sd, "decoder_tsdf.", c.reshape(B * M, 96).float(), pos_occ.reshape(B * M, 3))
        _, dc = R.head_backward(sd, "decoder_tsdf.", saved, dout.reshape(B * M, 1))
    return scatter_planes(pos_occ, dc)


def mismatches(got, ref):
    """Names of the compared values of `got` ({name: tensor}) that differ from the reference: bit for bit as numbers (-0 equals 0),
    except fc_p.weight's gradient in families B and C (ref.bounds)."""
    bad = []
    for k, want in ref.values.items():
        have = got[k].detach().cpu().reshape(want.shape)
        if k in ref.bounds:
            err = (have.double() - want.double()).abs()
            if bool((err > ref.bounds[k]).any()) or not bool(torch.isfinite(have).all()):
                bad.append((k, float(err.max()), float(ref.bounds[k].max())))
        elif bool((have != want).any()):
            n = int((have != want).sum())
            bad.append((k, n, have.numel(), float((have.double() - want.double()).abs().max())))
    return bad


# ---- harness: test-chosen planes in front of the training decoder kernels --------------------------------------------------------
def flat_params(sd, hp):
    """(flat fp32 parameters of head set hp in state-dict order, {name: shape})."""
    shapes = weights.giga_param_shapes(heads=heads_of(hp))
    return torch.cat([sd[k].reshape(-1).float() for k in shapes]), shapes


def run_decoder(sd, hp, detach, x, pos, pos_occ, douts, planes=None, dev=None, precision="bf16", around_backward=None):
    """One training step's decoder calls on the C entry points as training.GigaFunction drives them, on the host packer's blobs:
    giga_encoder_forward (fp32, so that the backward has its workspace), then -- with `planes` (3, B, 40, 40, 32), they replace
    the encoder's -- giga_decoder_forward (raw outputs of every head, then the training call) and giga_backward:
      "bf16"  the decoders in DEC_BF16, the backward with BF16_DECODER | BF16_CONVS | CONVIN_MASK_BWD (+ DETACH_OCC);
      "fp32"  the decoders at precision 0, the backward with CONVIN_MASK_BWD (+ DETACH_OCC) alone (csrc/giga_decoder_bwd.hip), and
              `qual`'s forward output replaced by 0.5 in what the backward reads (sigmoid' = 1/4 exactly: see the module docstring).
    Returns {name: CPU tensor}: raw/<head>, out/<head> (what the training call returned), grad/<param> of every decoder parameter,
    gplanes (3, B, 40, 40, 32) and planes (what the decoders sampled).  around_backward(call): runs instead of the one giga_backward
    call; call() enqueues giga_backward on the same buffers and waits for it, as often as it is asked to."""
    assert precision in PRECISIONS
    from giga_amd import _capi
    L = _capi.lib()
    dev = dev or torch.device("cuda:0")
    B, N = pos.shape[0], pos.shape[1]
    M = pos_occ.shape[1] if pos_occ is not None else 0
    flat, shapes = flat_params(sd, hp)
    res = {}
    with torch.cuda.device(dev):
        s = _capi.stream_ptr(dev)
        blob, bblob = _capi.pack_weights(flat, hp).to(dev), _capi.pack_bwd_weights(flat, hp).to(dev)
        ws = torch.empty(max(L.giga_encoder_workspace_bytes(B, 0), 16), dtype=torch.uint8, device=dev)
        nhwc = torch.empty((3, B, RES, RES, CD), device=dev, dtype=torch.float32)
        wsb = torch.empty(max(L.giga_backward_workspace_bytes(B, N, M, hp), 16), dtype=torch.uint8, device=dev)
        xd = x.contiguous().float().to(dev)
        _capi.check(L.giga_encoder_forward(_capi.ptr(xd), _capi.ptr(blob), _capi.ptr(nhwc), None, B, _capi.CONVIN_MASK,
                                           _capi.ptr(ws), ws.numel(), s), "giga_encoder_forward")
        if planes is not None:
            assert tuple(planes.shape) == tuple(nhwc.shape)
            nhwc.copy_(planes.to(dev))
        p = pos.contiguous().float().to(dev) if hp & 7 and N > 0 else None
        pt = pos_occ.contiguous().float().to(dev) if hp & 8 and M > 0 else None

        dec_precision = _capi.DEC_BF16 if precision == "bf16" else 0

        def forward(post):
            o = [torch.empty((B, N), device=dev) if hp & 1 and p is not None else None,
                 torch.empty((B, N, 4), device=dev) if hp & 2 and p is not None else None,
                 torch.empty((B, N), device=dev) if hp & 4 and p is not None else None,
                 torch.empty((B, M), device=dev) if pt is not None else None]
            if p is not None:
                _capi.check(L.giga_decoder_forward(_capi.ptr(nhwc), _capi.ptr(p), _capi.ptr(blob), hp & 7, _capi.ptr(o[0]),
                                                   _capi.ptr(o[1]), _capi.ptr(o[2]), None, B, N, dec_precision, post, s),
                            "giga_decoder_forward")
            if pt is not None:
                _capi.check(L.giga_decoder_forward(_capi.ptr(nhwc), _capi.ptr(pt), _capi.ptr(blob), 8, None, None, None,
                                                   _capi.ptr(o[3]), B, M, dec_precision, 0, s), "giga_decoder_forward")
            return o

        for h, t in zip(HEADS, forward(0)):
            if t is not None:
                res["raw/" + h] = t.cpu()
        outs = forward(1)
        for h, t in zip(HEADS, outs):
            if t is not None:
                res["out/" + h] = t.cpu()
        if precision == "fp32" and outs[0] is not None:
            outs[0].fill_(0.5)
        dd = [douts[h].contiguous().float().to(dev) if t is not None else None for h, t in zip(HEADS, outs)]
        arr_o, arr_d = (ctypes.c_void_p * 4)(), (ctypes.c_void_p * 4)()
        for i in range(4):
            arr_o[i] = outs[i].data_ptr() if outs[i] is not None else None
            arr_d[i] = dd[i].data_ptr() if dd[i] is not None else None
        grads = torch.empty(flat.numel(), device=dev, dtype=torch.float32)
        flags = hp | _capi.CONVIN_MASK_BWD | (_capi.DETACH_OCC if detach else 0)
        if precision == "bf16":
            flags |= _capi.BF16_DECODER | _capi.BF16_CONVS

        def backward():
            _capi.check(L.giga_backward(_capi.ptr(xd), _capi.ptr(blob), _capi.ptr(bblob), _capi.ptr(ws), _capi.ptr(nhwc), _capi.ptr(p),
                                        _capi.ptr(pt), arr_o, arr_d, _capi.ptr(grads), grads.numel(), flags, B, N, M, _capi.ptr(wsb),
                                        wsb.numel(), s), "giga_backward")
            torch.cuda.synchronize(dev)

        (around_backward or (lambda call: call()))(backward)
        gc, at = grads.cpu(), 0
        for k, shp in shapes.items():
            n = int(np.prod(shp))
            if k.startswith("decoder_"):
                res["grad/" + k] = gc[at:at + n].view(shp).clone()
            at += n
        res["gplanes"] = wsb[:3 * B * RES * RES * CD * 4].view(torch.float32).view(3, B, RES, RES, CD).cpu()
        res["planes"] = nhwc.cpu()
    return res


def run_bf16_decoder(sd, hp, detach, x, pos, pos_occ, douts, planes=None, dev=None):
    """run_decoder in "bf16"."""
    return run_decoder(sd, hp, detach, x, pos, pos_occ, douts, planes=planes, dev=dev, precision="bf16")
