"""Stage-by-stage float64 reference of the U-Net's backward: plain torch, no kernel knowledge.  Test infrastructure only
(tests/test_bwd_stage_host.py pins it to autograd on CPU; tests/test_gpu_bwd_stages.py holds the kernels to it).

The data-gradient chain is fifteen stages, in the order the backward runs them (csrc/giga_encoder_bwd.hip: the M.layer[] /
M.pool[] wiring of encoder_backward_impl; reference encoder/unet.py:225-239 reversed):

    L12 L11 L10 L9 L8 L7 L6 L5 L4 pool1 L3 L2 pool0 L1 L0

Buffers are NCHW tensors in a dict.  Gradient buffers carry the names of giga_backward_workspace_layout, g<X> = gradient of
the objective w.r.t. activation X of giga_encoder_workspace_layout with the ReLU mask of X already applied where X is a ReLU
output (gA6 gA5 gA4 gA3 gS2 gA2 gS1 gA1 gS0 gA0); gC1 / gC0 = w.r.t. the concatenated inputs (U | skip) of up1.conv1 /
up0.conv1; gOUT = w.r.t. the planes conv_final writes (the plane gradients the decoders leave).

Every stage function returns (want, mag): the float64 result, and the same expression on absolute values -- the sum of
|products| the accumulation noise of a kernel scales with.  `r` is an optional operand rounding, e.g. `bf16`, applied to
dY and W of a convolution stage (the bf16 step's kernels round both once and accumulate in fp32)."""
import collections

import torch
import torch.nn.functional as F

PREFIX = "encoder.unet."
# forward activations / gradient buffers: channels and edge length
ACT = {"P0": (32, 40), "A0": (32, 40), "S0": (32, 40), "Q0": (32, 20), "A1": (64, 20), "S1": (64, 20), "Q1": (64, 10),
       "A2": (128, 10), "S2": (128, 10), "U0": (64, 20), "A3": (64, 20), "A4": (64, 20), "U1": (32, 40), "A5": (32, 40),
       "A6": (32, 40)}
ACT_ORDER = ("P0", "A0", "S0", "Q0", "A1", "S1", "Q1", "A2", "S2", "U0", "A3", "A4", "U1", "A5", "A6")       # giga_encoder_workspace_layout
GRAD = {"gOUT": (32, 40), "gA6": (32, 40), "gA5": (32, 40), "gC1": (64, 40), "gA4": (64, 20), "gA3": (64, 20), "gC0": (128, 20),
        "gS2": (128, 10), "gA2": (128, 10), "gQ1": (64, 10), "gS1": (64, 20), "gA1": (64, 20), "gQ0": (32, 20), "gS0": (32, 40),
        "gA0": (32, 40), "gP0": (32, 40)}
GRAD_ORDER = ("gA6", "gA5", "gC1", "gA4", "gA3", "gC0", "gS2", "gA2", "gQ1", "gS1", "gA1", "gQ0", "gS0", "gA0", "gP0")   # giga_backward_workspace_layout

# kind: "conv3" (3x3, padding 1), "up" (ConvTranspose2d(k=2, s=2)), "conv1" (1x1), "pool" (MaxPool2d(2, 2) + skip add + ReLU).
# src / lo / hi: the input gradient buffer and its channel slice (a pool stage: the SKIP half of the concat gradient; its
# pooled gradient is `dq`).  key: the layer's weight.  mask: the forward activation whose > 0 mask applies to the output.
Stage = collections.namedtuple("Stage", "name kind src lo hi key dst mask dq")
STAGES = (
    Stage("L12", "conv1", "gOUT", 0, 32, "conv_final", "gA6", "A6", None),
    Stage("L11", "conv3", "gA6", 0, 32, "up_convs.1.conv2", "gA5", "A5", None),
    Stage("L10", "conv3", "gA5", 0, 32, "up_convs.1.conv1", "gC1", None, None),        # 64 channels out: (dU1 | dS0 skip part)
    Stage("L9", "up", "gC1", 0, 32, "up_convs.1.upconv", "gA4", "A4", None),
    Stage("L8", "conv3", "gA4", 0, 64, "up_convs.0.conv2", "gA3", "A3", None),
    Stage("L7", "conv3", "gA3", 0, 64, "up_convs.0.conv1", "gC0", None, None),         # 128 channels out: (dU0 | dS1 skip part)
    Stage("L6", "up", "gC0", 0, 64, "up_convs.0.upconv", "gS2", "S2", None),
    Stage("L5", "conv3", "gS2", 0, 128, "down_convs.2.conv2", "gA2", "A2", None),
    Stage("L4", "conv3", "gA2", 0, 128, "down_convs.2.conv1", "gQ1", None, None),
    Stage("pool1", "pool", "gC0", 64, 128, None, "gS1", "S1", "gQ1"),
    Stage("L3", "conv3", "gS1", 0, 64, "down_convs.1.conv2", "gA1", "A1", None),
    Stage("L2", "conv3", "gA1", 0, 64, "down_convs.1.conv1", "gQ0", None, None),
    Stage("pool0", "pool", "gC1", 32, 64, None, "gS0", "S0", "gQ0"),
    Stage("L1", "conv3", "gS0", 0, 32, "down_convs.0.conv2", "gA0", "A0", None),
    Stage("L0", "conv3", "gA0", 0, 32, "down_convs.0.conv1", "gP0", None, None),
)
STAGE = {s.name: s for s in STAGES}
CONV_STAGES = tuple(s for s in STAGES if s.kind != "pool")
# the weight gradients the layer-by-layer test of the 3x3 layers does not walk: (layer, kind, weight key, the layer's input
# activation, the buffer that holds the gradient of its output, channel slice of that buffer)
WGRADS = (("L6", "up", "up_convs.0.upconv", "S2", "gC0", 0, 64), ("L9", "up", "up_convs.1.upconv", "A4", "gC1", 0, 32),
          ("L12", "conv1", "conv_final", "A6", "gOUT", 0, 32))


def bf16(t):
    """Round to bfloat16 (nearest even) and back to the tensor's own type."""
    return t.bfloat16().to(t.dtype)


def _conv_dgrad(kind, dy, w):
    if kind == "conv3":
        return F.conv_transpose2d(dy, w, padding=1)          # = torch.nn.grad.conv2d_input: the transpose of conv2d(padding=1)
    if kind == "conv1":
        return F.conv_transpose2d(dy, w)
    return F.conv2d(dy, w, stride=2)                         # "up": the transpose of ConvTranspose2d(k = 2, s = 2), weight (cin, cout, 2, 2)


def conv_stage(st, dy, w, act=None, r=None):
    """(want, mag) of a convolution stage.  dy: the stage's input gradient buffer (all channels: the slice is taken here),
    w: the layer's weight, act: the activation named by st.mask (None: no mask)."""
    q = r if r is not None else (lambda t: t)
    dy = q(dy[:, st.lo:st.hi].double())
    w = q(w.double())
    want, mag = _conv_dgrad(st.kind, dy, w), _conv_dgrad(st.kind, dy.abs(), w.abs())
    if st.mask is not None:
        keep = act > 0
        want, mag = want * keep, mag * keep
    return want, mag


def first_max(s):
    """Boolean mask of s (N, C, H, W): the FIRST maximum of every 2x2 window in row-major order (torch's max_pool2d rule)."""
    n, c, h, w = s.shape
    win = s.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    eq = win == win.max(dim=-1, keepdim=True).values
    first = eq & (eq.cumsum(dim=-1) == 1)
    return first.reshape(n, c, h // 2, w // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h, w)


def upsample2(t):
    return t.repeat_interleave(2, -1).repeat_interleave(2, -2)


def pool_stage(st, dcat, dq, s):
    """(want, mag) of a pool stage, in the dtype of its inputs (fp32 buffers: one fp32 addition per element, so a kernel
    can be compared bit for bit):  dS = S > 0 ? dCat[:, lo:hi] + (first maximum of its window ? dQ : 0) : 0."""
    d = dcat[:, st.lo:st.hi]
    g = upsample2(dq)
    zero = torch.zeros_like(g)
    routed = torch.where(first_max(s), g, zero)
    keep = s > 0
    return torch.where(keep, d + routed, zero), torch.where(keep, d.abs() + routed.abs(), zero)


def stage_want(st, grads, acts, sd, r=None):
    """(want, mag) of stage `st` from the buffers that feed it: grads / acts are {name: NCHW tensor}, sd the state dict."""
    if st.kind == "pool":
        return pool_stage(st, grads[st.src], grads[st.dq], acts[st.mask])
    return conv_stage(st, grads[st.src], sd[PREFIX + st.key + ".weight"], acts[st.mask] if st.mask else None, r)


def wgrad_want(entry, grads, acts):
    """((dW, mag), (db, mag)) in float64 of one entry of WGRADS, operands unrounded:
    ConvTranspose2d: dW[ci][co][d] = sum over pixels p of In[p][ci] * dU[up(p, d)][co], db = column sums of dU over all
    four taps; conv_final: the 1x1 weight gradient, db = column sums of the plane gradients."""
    _, kind, _, xin, src, lo, hi = entry
    x, dy = acts[xin].double(), grads[src][:, lo:hi].double()
    if kind == "up":
        shape = (x.shape[1], dy.shape[1], 2, 2)
        f = lambda a, b: torch.nn.grad.conv2d_weight(b, shape, a, stride=2)  # noqa: E731  (the weight of conv2d(dU, W, stride 2) = dIn)
    else:
        shape = (dy.shape[1], x.shape[1], 1, 1)
        f = lambda a, b: torch.nn.grad.conv2d_weight(a, shape, b)  # noqa: E731
    return (f(x, dy), f(x.abs(), dy.abs())), (dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)))


# ---- tolerances (tests/test_gpu_bwd_stages.py; tests/test_bwd_stage_host.py shows what they reject) -------------------
def tol_bf16(want, mag):
    """Per-element bound of a bf16 convolution stage against the reference on bf16-rounded operands, and of the fp32-MFMA
    weight gradients against unrounded operands: the bound of test_bf16_weight_gradient_kernels_with_rounded_operands."""
    return 2e-5 * float(want.abs().max()) + 1e-5 * mag


def tol_fp32(want, mag=None):
    """Bound of an fp32 convolution stage (Winograd, direct, persistent): tests/test_gpu_wino.py: TOL of the tensor's max."""
    return torch.full_like(want, 2e-5 * float(want.abs().max()))
