"""Numpy restatement of the epoch accumulator of giga_train_loss_metrics (include/giga_hip.h, csrc/giga_loss.hip) and of the
metrics made from it (ignite's binary Accuracy / Precision / Recall and Average as scripts/train_giga.py:53-59 configures them),
written from the definitions, for the GPU tests of giga_amd.trainer."""
import numpy as np

WORDS = 16
COUNTS = ("batches", "examples", "correct", "tp", "fp", "fn", "invalid")            # words 0-6, uint64
SUM_WORD = 8                                                                         # words 8-12, double
LOSS_ORDER = ("loss_qual", "loss_rot", "loss_width", "loss_occ", "loss_all")        # scene_losses' columns
KEYS = ("accuracy", "precision", "recall", "loss_all", "loss_qual", "loss_rot", "loss_width", "loss_occ")


def update(words, qual, label, losses):
    """one call: `words` (16 uint64) -> the words after a batch with quality outputs `qual`, labels `label` (float32, one per
    scene) and batch means `losses` (5 float32).  Words 7 and 13-15 pass through."""
    w = np.array(words, dtype=np.uint64).copy()
    assert w.shape == (WORDS,)
    q, y = np.asarray(qual, np.float32).reshape(-1), np.asarray(label, np.float32).reshape(-1)
    assert q.shape == y.shape and len(q) >= 1
    with np.errstate(invalid="ignore"):
        valid = (q >= 0) & (q <= 1) & ((y == 0) | (y == 1))          # a NaN compares false
        pred = q > np.float32(0.5)                                   # torch.round: half to even, 0.5 -> 0
    pos = y == 1
    add = dict(batches=1, examples=valid.sum(), correct=(valid & (pred == pos)).sum(), tp=(valid & pred & pos).sum(),
               fp=(valid & pred & ~pos).sum(), fn=(valid & ~pred & pos).sum(), invalid=(~valid).sum())
    for i, k in enumerate(COUNTS):
        w[i] += np.uint64(int(add[k]))
    sums = w.view(np.float64)
    for k, v in enumerate(np.asarray(losses, np.float32).reshape(5)):
        sums[SUM_WORD + k] = sums[SUM_WORD + k] + np.float64(v)     # one float64 addition of the fp32 mean per call
    return w


def finalize(words):
    """the reference's dictionary from the words, float64 throughout"""
    w = np.asarray(words).view(np.uint64)
    c = {k: int(w[i]) for i, k in enumerate(COUNTS)}
    sums = np.asarray(words).view(np.float64)[SUM_WORD:SUM_WORD + 5]
    assert c["batches"] > 0 and c["invalid"] == 0
    out = {"accuracy": c["correct"] / c["examples"], "precision": c["tp"] / (c["tp"] + c["fp"] + 1e-20),
           "recall": c["tp"] / (c["tp"] + c["fn"] + 1e-20)}
    for k, s in zip(LOSS_ORDER, sums):
        out[k] = float(s) / c["batches"]
    return {k: float(out[k]) for k in KEYS}


def edge_quals(n, rng):
    """n sigmoid-range values that include 0, 1, exactly 0.5 and its two float32 neighbours (as far as n allows)"""
    half = np.float32(0.5)
    edges = np.array([0.0, 1.0, half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0))], np.float32)
    q = rng.random(n, dtype=np.float32)
    k = min(n, len(edges))
    q[rng.permutation(n)[:k]] = rng.permutation(edges)[:k]
    return q
