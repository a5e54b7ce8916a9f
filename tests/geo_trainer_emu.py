"""Numpy restatement of the epoch accumulator of giga_train_occ_loss_metrics (include/giga_hip.h, csrc/giga_loss.hip) and of the
metrics made from it (an Average of the loss and ignite's binary Accuracy / Precision / Recall over every occupancy point, as
scripts/train_giga_geo.py:52-57 configures them), written from the definitions, for the tests of giga_amd.trainer.GeoTrainer."""
import numpy as np

WORDS = 16
COUNTS = ("batches", "examples", "correct", "tp", "fp", "fn", "invalid")            # words 0-6, uint64; all but the first in points
SUM_WORD = 8                                                                         # doubles from word 8 on
LOSS_WORDS = (SUM_WORD + 3, SUM_WORD + 4)                                            # both take (double)loss: loss_occ and loss_all
KEYS = ("loss", "occ_accuracy", "occ_precision", "occ_recall")


def probabilities(logits, band="refuse"):
    """float32 sigmoid as far as the classification needs it: NaN stays NaN, and p > 0.5 exactly where z > 0 for every logit with
    z == 0 or |z| >= 1e-6 (1 + exp(-z) is then 2 or at least four float32 steps from it, whatever the last bit of exp).  Logits
    with 0 < |z| < 1e-6 are refused: there the rounding of exp decides.  band="float32" evaluates those in numpy's float32
    instead, for logits a test does not choose (a network's outputs): 1 / (1 + exp(-z)) with each step rounded, which is the
    kernel's value wherever the two exps round alike."""
    z = np.asarray(logits, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        inside = (np.abs(z) > 0) & (np.abs(z) < np.float32(1e-6))
        assert band == "float32" or not inside.any()
        p = np.where(z > 0, np.float32(0.75), np.float32(0.25)).astype(np.float32)
        p[z == 0] = np.float32(0.5)                                  # 1 / (1 + 1): exactly one half, which rounds to 0
        p[inside] = np.float32(1) / (np.float32(1) + np.exp(-z[inside], dtype=np.float32))
    p[np.isnan(z)] = np.nan
    return p


def update(words, logits, target, loss, band="refuse"):
    """one call: `words` (16 uint64) -> the words after a batch with occupancy logits `logits` and targets `target` ((B, M)
    float32) and the batch's loss (one float32).  Words 7, 8-10 and 13-15 pass through."""
    w = np.array(words, dtype=np.uint64).copy()
    assert w.shape == (WORDS,)
    p, t = probabilities(logits, band).reshape(-1), np.asarray(target, np.float32).reshape(-1)
    assert p.shape == t.shape and len(p) >= 1
    with np.errstate(invalid="ignore"):
        valid = ~np.isnan(p) & ((t == 0) | (t == 1))
        pred = p > np.float32(0.5)                                   # torch.round: half to even, 0.5 -> 0
    pos = t == 1
    add = dict(batches=1, examples=valid.sum(), correct=(valid & (pred == pos)).sum(), tp=(valid & pred & pos).sum(),
               fp=(valid & pred & ~pos).sum(), fn=(valid & ~pred & pos).sum(), invalid=(~valid).sum())
    for i, k in enumerate(COUNTS):
        w[i] += np.uint64(int(add[k]))
    sums = w.view(np.float64)
    for k in LOSS_WORDS:
        sums[k] = sums[k] + np.float64(np.float32(loss))             # one float64 addition of the fp32 mean per call
    return w


def finalize(words):
    """the reference's dictionary from the words, float64 throughout"""
    w = np.asarray(words).view(np.uint64)
    c = {k: int(w[i]) for i, k in enumerate(COUNTS)}
    assert c["batches"] > 0 and c["invalid"] == 0
    return {"loss": float(np.asarray(words).view(np.float64)[LOSS_WORDS[0]]) / c["batches"],
            "occ_accuracy": c["correct"] / c["examples"],
            "occ_precision": c["tp"] / (c["tp"] + c["fp"] + 1e-20),
            "occ_recall": c["tp"] / (c["tp"] + c["fn"] + 1e-20)}


def edge_logits(shape, rng, scale=3.0):
    """float32 logits of `shape` with the edge values +-0.0, +-1e-6, +-120 and +-inf among them (as far as the size allows) and no
    value with 0 < |z| < 1e-6"""
    z = (rng.standard_normal(shape) * scale).astype(np.float32)
    small = np.abs(z) < np.float32(1e-6)
    z[small] = np.float32(1e-6)
    edges = np.array([0.0, -0.0, 1e-6, -1e-6, 120.0, -120.0, np.inf, -np.inf], np.float32)
    flat = z.reshape(-1)
    k = min(flat.size, len(edges))
    flat[rng.permutation(flat.size)[:k]] = rng.permutation(edges)[:k]
    return flat.reshape(shape)
