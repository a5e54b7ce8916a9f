"""Float64 reference of the forward path, the weight / input families the envelope tests sweep, and the range-relative
comparison they use.  Test infrastructure only (tests/test_ref64.py pins it on CPU; tests/test_gpu_envelope.py and
tests/test_gpu_batch_limits.py hold the kernels to it).

The encoder is oracle.giga_oracle's, run on a float64 state dict.  The heads are tests/pgrad_ref.py's mlp64 on features
sampled in float64 at the coordinates the kernels use: normalize_coordinate in fp32 on the fp32 points (its clamps and the
reference's 1 + 10e-6 divisor are fp32 decisions), everything after it in float64.

train_grads is the training step's float64 reference (parameter gradients by autograd through the same chain;
tests/test_ref64_backward.py pins it, tests/test_gpu_backward_envelope.py holds the backward kernels to it), and census
counts the near-ties where fp32 and float64 may legitimately route a gradient differently."""
import contextlib

import numpy as np
import torch
import torch.nn.functional as F

from giga_amd import synth, weights
from oracle import giga_oracle as O
from pgrad_ref import mlp64

HEADS = ("decoder_qual", "decoder_rot", "decoder_width", "decoder_tsdf")
WEIGHT_FAMILIES = ("he-7", "he-11", "he-23", "spread", "nobias")
INPUT_FAMILIES = ("uniform", "realistic", "structured", "adversarial")
# Range-relative tolerance of the fp32-class modes against float64: 2x the worst measured on an MI355X over every family,
# form and output of tests/test_gpu_envelope.py (fp32 1.75e-5: 'spread' rot, direct convolutions; fp16x3 1.6e-5: 'nobias'
# planes of the single-voxel scene, values under 2^-3 where the split loses relative precision).  Bounded above by the
# sensitivity check (tests/test_ref64.py: one U-Net layer with f16 operands moves the planes by >= 4x this; the least
# sensitive layer, up_convs.0.upconv, by 1.56e-4).
TOL = {"fp32": 3.5e-5, "fp16x3": 3.5e-5}
# Per-parameter-tensor tolerance of the fp32 training step against train_grads (max |got - ref| / max |ref|): see
# tests/test_gpu_backward_envelope.py for the measured worst, tests/test_ref64_backward.py for what it rejects.
TOL_BWD = 1.25e-4


# ---- float64 reference ---------------------------------------------------------------------------------------------
def sd64(sd):
    return {k: torch.as_tensor(v).double() for k, v in sd.items()}


def encoder(sd, x):
    """Planes {'xz','xy','yz'}: (B,32,40,40) float64 of x (B,40,40,40)."""
    with torch.no_grad():
        return O.encoder_forward(sd64(sd), torch.as_tensor(x).double())


def sample_features(p, planes):
    """(B,N,96) float64: oracle.sample_features with the coordinate normalisation in fp32."""
    p32 = torch.as_tensor(p).float()
    cols = []
    for k in O.PLANES:
        xy = O.normalize_coordinate(p32, k).double()
        vgrid = 2.0 * xy[:, :, None] - 1.0
        cols.append(F.grid_sample(planes[k].double(), vgrid, padding_mode="border", align_corners=True,
                                  mode="bilinear").squeeze(-1))
    return torch.cat(cols, dim=1).transpose(1, 2)


def heads(sd, planes, p, names=HEADS):
    """(raw, out): raw logits and epilogued outputs (sigmoid qual, unit rot, raw width / tsdf) of `names` at p, float64."""
    sd = sd64(sd)
    with torch.no_grad():
        c = sample_features(p, planes)
        p64 = torch.as_tensor(p).double()
        raw, out = {}, {}
        for h in names:
            z = mlp64(sd, h, p64, c)
            raw[h] = z
            out[h] = torch.sigmoid(z) if h == "decoder_qual" else F.normalize(z, dim=2) if h == "decoder_rot" else z
    return raw, out


# ---- comparison ----------------------------------------------------------------------------------------------------
def range_err(got, ref):
    """max |got - ref| / range(ref) of ONE scene's output (any shape); inf when got has a non-finite entry."""
    g = torch.as_tensor(got).double().cpu()
    r = torch.as_tensor(ref).double().cpu()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    rng = (r.max() - r.min()).item()
    return (g - r).abs().max().item() / max(rng, 1e-30)


def finite_err(got, ref):
    """(max |got - ref| / range(ref) over the FINITE entries of got, number of non-finite entries): the rule past the
    f16 range, where an entry must be either right or visibly wrong (NaN / inf), never a finite wrong number."""
    g = torch.as_tensor(got).double().cpu()
    r = torch.as_tensor(ref).double().cpu()
    fin = torch.isfinite(g)
    rng = max((r.max() - r.min()).item(), 1e-30)
    e = (g - r).abs()[fin].max().item() / rng if bool(fin.any()) else 0.0
    return e, int((~fin).sum())


def rot_err(got, ref, raw, finite_only=False):
    """range_err of unit quaternions with each point's error weighted by |raw_i| / max |raw|: the L2 normalisation divides
    an operand error by |raw|, so this is the raw-logit-scale error (points with a near-zero raw vector are ill-posed).
    finite_only: like finite_err, over the points whose quaternion is finite; returns (error, non-finite entries)."""
    g = torch.as_tensor(got).double().cpu()
    fin = torch.isfinite(g).all(dim=-1)
    if not finite_only and not bool(fin.all()):
        return float("inf")
    n = torch.as_tensor(raw).double().norm(dim=-1, keepdim=True)
    w = ((g - ref).abs() * n / n.max())[fin]
    e = (w.max().item() if w.numel() else 0.0) / max((ref.max() - ref.min()).item(), 1e-30)
    return (e, int((~torch.isfinite(g)).sum())) if finite_only else e


def planes_err(got, ref, k):
    """Worst range_err over the three planes of scene k; `got` / `ref` are plane dicts of batches that hold scene k."""
    return max(range_err(got[key][k], ref[key][k]) for key in O.PLANES)


# ---- weight families -----------------------------------------------------------------------------------------------
def weight_family_numpy(name):
    """{name: float32 ndarray} of a weight family:
    he-<seed>  the builder's He-uniform weights;
    spread     he-7 with per-output-channel gains log-uniform in [1/4, 4] and biases U[-0.5, 0.5] (a stand-in for trained
               weights: channels of very different magnitude, biases that are not small);
    nobias     he-7 with every bias zero;
    nobias-nofcp  nobias with every fc_p weight zero too (the decoders are then homogeneous in the planes)."""
    if name.startswith("he-"):
        return weights.make_state_dict_numpy(int(name[3:]))
    sd = weights.make_state_dict_numpy(7)
    if name == "spread":
        rng = np.random.default_rng(2024)
        out = {}
        for k, v in sd.items():
            if k.endswith("bias"):
                out[k] = rng.uniform(-0.5, 0.5, size=v.shape).astype(np.float32)
                continue
            # output channel axis: dim 1 of a ConvTranspose2d weight (Cin, Cout, 2, 2), dim 0 of every other weight
            axis = 1 if k.endswith("upconv.weight") else 0
            g = np.exp(rng.uniform(np.log(0.25), np.log(4.0), size=v.shape[axis])).astype(np.float32)
            shape = [1] * v.ndim
            shape[axis] = v.shape[axis]
            out[k] = (v * g.reshape(shape)).astype(np.float32)
        return out
    if name in ("nobias", "nobias-nofcp"):
        out = {k: (np.zeros_like(v) if k.endswith("bias") else v) for k, v in sd.items()}
        if name == "nobias-nofcp":
            out = {k: (np.zeros_like(v) if ".fc_p." in k else v) for k, v in out.items()}
        return out
    raise ValueError(name)


def weight_family(name):
    return {k: torch.from_numpy(v) for k, v in weight_family_numpy(name).items()}


# ---- input families ------------------------------------------------------------------------------------------------
def _structured_scene(seed):
    """Truncated-distance TSDF in [0, 1] of a few boxes and spheres: smooth fields, large constant regions (0 far outside,
    1 deep inside after truncation) and sharp bands at the surfaces."""
    rng = np.random.default_rng(9000 + seed)
    g = (np.arange(40, dtype=np.float64) + 0.5) / 40 - 0.5
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    sdf = np.full(X.shape, 1e9)
    for _ in range(int(rng.integers(2, 5))):
        c = rng.uniform(-0.3, 0.3, 3)
        if rng.random() < 0.5:
            d = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - rng.uniform(0.05, 0.2)
        else:
            h = rng.uniform(0.04, 0.18, 3)
            q = np.stack([np.abs(X - c[0]) - h[0], np.abs(Y - c[1]) - h[1], np.abs(Z - c[2]) - h[2]])
            d = np.linalg.norm(np.maximum(q, 0), axis=0) + np.minimum(q.max(0), 0)
        sdf = np.minimum(sdf, d)
    trunc = 4.0 / 40
    t = np.clip(-sdf / trunc, -1.0, 1.0)             # +1 inside, -1 outside, linear across a 4-voxel band
    return np.where(t <= -1.0, 0.0, 0.5 * (t + 1.0)).astype(np.float32)


def adversarial_scenes():
    """The four scenes of the encoder fuzz test: empty, all ones, a single voxel (plus a half at the far corner), checkerboard."""
    x = np.zeros((4, 40, 40, 40), np.float32)
    x[1] = 1.0
    x[2, 0, 0, 0] = 1.0
    x[2, 39, 39, 39] = 0.5
    g = np.arange(40)
    x[3] = ((g[:, None, None] + g[None, :, None] + g[None, None, :]) % 2).astype(np.float32)
    return x


def input_family(name, B, first=0):
    """(B,40,40,40) float32 TSDFs of an input family; every scene differs from the others (adversarial: the four scenes
    first, then uniform ones)."""
    if name == "uniform":
        return synth.tsdf_batch(first, B)
    if name == "realistic":
        return synth.tsdf_batch(first, B, realistic=True)
    if name == "structured":
        return np.stack([_structured_scene(first + i) for i in range(B)])
    if name == "adversarial":
        adv = adversarial_scenes()
        if B <= 4:
            return adv[:B].copy()
        return np.concatenate([adv, synth.tsdf_batch(first + 4, B - 4)])
    raise ValueError(name)


# ---- f16x3 split (precision 2) -------------------------------------------------------------------------------------
def f16x3_split(v):
    """hi = f16(v), lo = f16(v - hi) in numpy (round to nearest even, as v_cvt_f16_f32); returns (hi, lo) as float32."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = v.astype(np.float16)
        lo = (v - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float32), lo.astype(np.float32)


# ---- float64 training reference --------------------------------------------------------------------------------------
def head_keys(sd, heads):
    """The state-dict keys of a model with `heads` (encoder + those heads), in state-dict order."""
    return [k for k in sd if k.startswith("encoder.") or k.split(".")[0] in heads]


def smooth_objective(B, N, M, heads=HEADS, seed=0):
    """{head: R} of the smooth objective sum_h <out_h, R_h>: fixed N(0, 1) weights scaled by 1 / (points per scene), so
    every head's share is O(1).  Unlike the training loss it has no saturating term: every output carries gradient."""
    g = torch.Generator().manual_seed(seed)
    shape = {"decoder_qual": (B, N), "decoder_rot": (B, N, 4), "decoder_width": (B, N), "decoder_tsdf": (B, M)}
    return {h: torch.randn(shape[h], generator=g, dtype=torch.float64) / max(1, shape[h][1]) for h in heads}


def train_outputs(sd, x, pos, pos_occ, heads=HEADS, detach_tsdf=False):
    """{head: output} of the model forward (models/__init__.py:42-67) in the dtype of `sd`: sigmoid qual, unit rot, raw width
    at pos; raw occupancy logits at pos_occ (planes detached first when detach_tsdf).  Coordinates normalised in fp32."""
    dt = next(iter(sd.values())).dtype
    planes = O.encoder_forward(sd, torch.as_tensor(x).to(dt))
    out = {}
    for h in heads:
        p = pos_occ if h == "decoder_tsdf" else pos
        pl = {k: v.detach() for k, v in planes.items()} if h == "decoder_tsdf" and detach_tsdf else planes
        c = sample_features(p, pl).to(dt)
        z = mlp64(sd, h, torch.as_tensor(p).to(dt), c)
        out[h] = torch.sigmoid(z) if h == "decoder_qual" else F.normalize(z, dim=2) if h == "decoder_rot" else z
    return out


def train_grads(sd, x, pos, pos_occ, y=None, heads=HEADS, detach_tsdf=False, objective="loss", dtype=torch.float64):
    """(parts, grads) of one training step, by autograd in float64 (or `dtype`) through train_outputs.
    objective "loss": the joint loss O.train_loss(O.train_select(out), y) (all four heads, one grasp query per scene);
    parts = its five terms.  objective {head: R}: sum_h <out_h, R_h> (smooth_objective); parts = {"objective": value}.
    grads: {key: gradient} of every parameter of the model with `heads`."""
    sdg = {k: torch.as_tensor(sd[k]).to(dtype).clone().requires_grad_(True) for k in head_keys(sd, heads)}
    out = train_outputs(sdg, x, pos, pos_occ, heads, detach_tsdf)
    if isinstance(objective, str):
        assert objective == "loss" and tuple(heads) == HEADS, objective
        loss, d = O.train_loss(O.train_select(tuple(out[h] for h in HEADS)), tuple(torch.as_tensor(t).to(dtype) for t in y))
        parts = {k: v.item() for k, v in d.items()}
    else:
        loss = sum((out[h] * objective[h].to(dtype)).sum() for h in heads)
        parts = {"objective": loss.item()}
    loss.backward()
    return parts, {k: v.grad for k, v in sdg.items()}


def grad_err(got, ref):
    """max |got - ref| / max |ref| of one parameter tensor (inf when got has a non-finite entry)."""
    g = torch.as_tensor(got).double().cpu()
    r = torch.as_tensor(ref).double().cpu()
    if not bool(torch.isfinite(g).all()):
        return float("inf")
    return (g - r).abs().max().item() / max(r.abs().max().item(), 1e-30)


@contextlib.contextmanager
def patched_functional(**fns):
    """Replace torch.nn.functional.<name> for the duration (the oracle and mlp64 look them up at call time): the census'
    recorders and the sensitivity tests' mutated operators."""
    saved = {k: getattr(F, k) for k in fns}
    try:
        for k, v in fns.items():
            setattr(F, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(F, k, v)


def census(sd, x, pos=None, pos_occ=None, heads=HEADS, rel=1e-6):
    """Near-ties of one case's float64 forward, where the kernels' fp32 may legitimately route a gradient otherwise:
    pool_near_ties  2x2 max-pool windows whose two largest values are both positive and 0 < gap <= rel * range(pool input);
    pool_ties       windows whose maximum is positive and held by >= 2 elements exactly (routed by the tie rule);
    relu_near_zero  ReLU inputs with 0 < |z| <= rel * range(that ReLU's input);
    relu_zero       ReLU inputs exactly 0 (whose gradient the ReLU's strict '>' drops)."""
    n = {"pool_near_ties": 0, "pool_ties": 0, "relu_near_zero": 0, "relu_zero": 0}
    relu, pool = F.relu, F.max_pool2d

    def rec_relu(z, *a, **k):
        rng = (z.max() - z.min()).item()
        n["relu_near_zero"] += int(((z != 0) & (z.abs() <= rel * rng)).sum())
        n["relu_zero"] += int((z == 0).sum())
        return relu(z, *a, **k)

    def rec_pool(s, *a, **k):
        B, C, H, W = s.shape
        w = s.reshape(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4)
        t = w.topk(2, dim=1).values
        gap, rng = t[:, 0] - t[:, 1], (s.max() - s.min()).item()
        n["pool_near_ties"] += int(((t[:, 1] > 0) & (gap > 0) & (gap <= rel * rng)).sum())
        n["pool_ties"] += int(((t[:, 0] > 0) & (gap == 0)).sum())
        return pool(s, *a, **k)

    sd = {k: torch.as_tensor(sd[k]).double() for k in head_keys(sd, heads)}
    with torch.no_grad(), patched_functional(relu=rec_relu, max_pool2d=rec_pool):
        planes = O.encoder_forward(sd, torch.as_tensor(x).double())
        for h in heads:
            p = pos_occ if h == "decoder_tsdf" else pos
            if p is not None and p.shape[1] > 0:
                mlp64(sd, h, torch.as_tensor(p).double(), sample_features(p, planes))
    return n
