"""The training loop of the reference's scripts/train_giga.py on the pieces of this package: epochs over `ResidentBatches`, the
fused loss, `FlatAdam`, ignite's epoch metrics, the validation pass and the two rotating checkpoints.

An epoch runs without the host waiting for the device: the metrics of a step are accumulated on the device by the loss launch
itself (`giga_train_loss_metrics`, csrc/giga_loss.hip) into the 128 bytes a `TrainMetrics` owns, and an epoch ends with one
small device-to-host copy.

    rset = ResidentTrainingSet(GraspOccDataset(root, raw))
    train_idx, val_idx = train_val_split(len(rset), 0.1, seed=0)
    trainer = Trainer(net, ResidentBatches(rset, 32, drop_last=True, indices=train_idx),
                      ResidentBatches(rset, 32, shuffle=False, drop_last=True, indices=val_idx), logdir="runs/a", precision="bf16")
    records = trainer.run(10)

The files in `logdir` are the reference's: `vgn_<net>_<iteration>.pt` after every epoch and `best_vgn_<net>_val_acc=<acc>.pt` for
the best validation accuracy, both plain state dicts that `load_network` reads; beside them `trainer_state.pt` (what `resume=True`
needs) and `metrics.jsonl` (one line per epoch).  Device tensors only; no CPU fallback.

`GeoTrainer` is the same loop for the occupancy-only `giga_geo` (the reference's scripts/train_giga_geo.py):
`geo_loss` in place of `giga_loss`, the metrics `loss`, `occ_accuracy`, `occ_precision`, `occ_recall` counted over every occupancy
point by the loss launch (`giga_train_occ_loss_metrics`) into the same 128 bytes, `python -m giga_amd.train_geo`."""
import glob
import itertools
import json
import os

import numpy as np
import torch

from . import _capi
from .optim import FlatAdam
from .training import LOSS_KEYS, allreduce_mean_, geo_loss, giga_loss

WORDS = _capi.TRAIN_METRICS_BYTES // 8                      # sixteen 8-byte words (include/giga_hip.h)
COUNT_NAMES = ("batches", "examples", "correct", "tp", "fp", "fn", "invalid")       # words 0-6, uint64
SUM_WORD = 8                                                 # words 8-12, double: running sums of the batch means, LOSS_KEYS' order
METRIC_KEYS = ("accuracy", "precision", "recall", "loss_all", "loss_qual", "loss_rot", "loss_width", "loss_occ")    # train_giga.py:53-59
NETS = ("giga", "giga_detach", "giga_aff")
GEO_METRIC_KEYS = ("loss", "occ_accuracy", "occ_precision", "occ_recall")          # train_giga_geo.py:52-57


def finalize_metrics(words):
    """The reference's epoch metrics (ignite's binary Accuracy, Precision, Recall and five Averages as train_giga.py:53-59
    configures them) from the sixteen accumulator words, in float64 -> dict with METRIC_KEYS.  ValueError for an accumulator
    that saw no batch, and for one that counted scenes whose prediction or label is not binary (ignite raises there too)."""
    raw = np.ascontiguousarray(np.asarray(words)).reshape(-1)
    if raw.size != WORDS or raw.dtype.itemsize != 8:
        raise ValueError(f"the accumulator is {WORDS} 8-byte words")
    c = dict(zip(COUNT_NAMES, (int(v) for v in raw.view(np.uint64)[:len(COUNT_NAMES)])))
    sums = raw.view(np.float64)[SUM_WORD:SUM_WORD + len(LOSS_KEYS)]
    if c["batches"] == 0:
        raise ValueError("the metrics of an epoch need at least one batch")
    if c["invalid"] > 0:
        raise ValueError(f"{c['invalid']} scenes with a quality outside [0, 1] or a label other than 0 and 1: binary metrics are "
                         "not defined for them")
    f = np.float64
    out = {"accuracy": f(c["correct"]) / f(c["examples"]),
           "precision": f(c["tp"]) / (f(c["tp"] + c["fp"]) + f(1e-20)),
           "recall": f(c["tp"]) / (f(c["tp"] + c["fn"]) + f(1e-20))}
    for k, s in zip(LOSS_KEYS, sums):
        out[k] = f(s) / f(c["batches"])
    return {k: float(out[k]) for k in METRIC_KEYS}


def finalize_geo_metrics(words):
    """The epoch metrics of the reference's train_giga_geo.py:52-57 (an Average of the loss and ignite's binary Accuracy, Precision
    and Recall over every occupancy point of the epoch) from the sixteen accumulator words as `geo_loss(..., metrics=m)` fills them,
    in float64 -> dict with GEO_METRIC_KEYS.  The counts are points, not scenes; the loss is the sum in word 8 + 3 (the occupancy
    mean, which is the whole objective) over the batches.  ValueError for an accumulator that saw no batch, and for one that counted
    points whose probability is NaN or whose target is not 0 or 1 (ignite raises there too)."""
    raw = np.ascontiguousarray(np.asarray(words)).reshape(-1)
    if raw.size != WORDS or raw.dtype.itemsize != 8:
        raise ValueError(f"the accumulator is {WORDS} 8-byte words")
    c = dict(zip(COUNT_NAMES, (int(v) for v in raw.view(np.uint64)[:len(COUNT_NAMES)])))
    if c["batches"] == 0:
        raise ValueError("the metrics of an epoch need at least one batch")
    if c["invalid"] > 0:
        raise ValueError(f"{c['invalid']} points with a NaN probability or a target other than 0 and 1: binary metrics are not "
                         "defined for them")
    f = np.float64
    out = {"loss": f(raw.view(np.float64)[SUM_WORD + LOSS_KEYS.index("loss_occ")]) / f(c["batches"]),
           "occ_accuracy": f(c["correct"]) / f(c["examples"]),
           "occ_precision": f(c["tp"]) / (f(c["tp"] + c["fp"]) + f(1e-20)),
           "occ_recall": f(c["tp"]) / (f(c["tp"] + c["fn"]) + f(1e-20))}
    return {k: float(out[k]) for k in GEO_METRIC_KEYS}


def all_reduce_words_(acc, group=None):
    """Sum the counts (int64) and the running sums (float64) of an accumulator tensor over the ranks of `group`, in place; the
    reserved words stay.  No-op when torch.distributed is not initialised."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(acc[:len(COUNT_NAMES)], op=dist.ReduceOp.SUM, group=group)
        dist.all_reduce(acc[SUM_WORD:SUM_WORD + len(LOSS_KEYS)].view(torch.float64), op=dist.ReduceOp.SUM, group=group)
    return acc


class TrainMetrics:
    """The epoch accumulator of `giga_loss(..., metrics=m)`: 128 bytes of device memory (sixteen int64 words; layout in
    include/giga_hip.h), updated by the loss launch of every step."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise _capi.GigaHipError(f"training metrics live on a HIP device, not on {device}; there is no CPU fallback")
        self.acc = torch.zeros(WORDS, dtype=torch.int64, device=device)

    def reset(self):
        """zero the accumulator, asynchronously on the current stream"""
        self.acc.zero_()
        return self

    def all_reduce(self, group=None):
        all_reduce_words_(self.acc, group)
        return self

    def words(self):
        """the one device-to-host copy -> sixteen int64 words (numpy)"""
        return self.acc.cpu().numpy()

    def compute(self):
        return finalize_metrics(self.words())


def train_val_split(n, val_split, seed=0):
    """(train_indices, val_indices) of n grasp rows: val_size = int(val_split * n) as create_train_val_loaders
    (train_giga.py:128-130); the order is `default_rng([seed, 0]).permutation(n)`, its first n - val_size entries are the train
    rows.  (The reference's `random_split` draws from torch's global generator; this split is the package's own, in the style of
    `resident.epoch_order`.)"""
    n = int(n)
    val_size = int(val_split * n)
    if n < 0 or not 0 <= val_size <= n:
        raise ValueError("val_split lies in [0, 1]")
    order = np.random.default_rng([int(seed), 0]).permutation(n).astype(np.int64)
    return order[:n - val_size], order[n - val_size:]


class Checkpoints:
    """The files of a run directory, as ignite's two `ModelCheckpoint(n_saved=1, require_empty=True)` of train_giga.py:98-117
    leave them: one `vgn_<net>_<iteration>.pt`, one `best_vgn_<net>_val_acc=<acc>.pt`, both plain state dicts."""

    def __init__(self, logdir, net_name, resume=False):
        self.dir, self.net_name = str(logdir), net_name
        os.makedirs(self.dir, exist_ok=True)
        if not resume and glob.glob(os.path.join(glob.escape(self.dir), "*.pt")):
            raise ValueError(f"{self.dir} already holds checkpoint files; pass resume=True to continue that run")
        self.best_score = None
        self.state_path = os.path.join(self.dir, "trainer_state.pt")

    def _write(self, obj, name, pattern=None):
        """`torch.save(obj)` as `name`, complete or not at all (a temporary file, then `os.replace`); with `pattern`, the other
        files that match it go once the new one is there -> the path"""
        path = os.path.join(self.dir, name)
        torch.save(obj, path + ".tmp")
        os.replace(path + ".tmp", path)
        if pattern is not None:
            for old in glob.glob(os.path.join(glob.escape(self.dir), pattern)):
                if os.path.abspath(old) != os.path.abspath(path):
                    os.remove(old)
        return path

    def epoch_files(self):
        """[(iteration, path)] of the `vgn_<net>_<iteration>.pt` files of the directory, oldest iteration first"""
        prefix = f"vgn_{self.net_name}_"
        found = []
        for path in glob.glob(os.path.join(glob.escape(self.dir), prefix + "*.pt")):
            stem = os.path.basename(path)[len(prefix):-3]
            if stem.isdigit():
                found.append((int(stem), path))
        return sorted(found)

    def save_epoch(self, state_dict, iteration):
        return self._write(state_dict, f"vgn_{self.net_name}_{int(iteration)}.pt", f"vgn_{self.net_name}_[0-9]*.pt")

    def save_best(self, state_dict, score):
        """write the "best" file when `score` is strictly greater than every score before -> its path, else None"""
        score = float(score)
        if self.best_score is not None and not score > self.best_score:
            return None
        self.best_score = score
        return self._write(state_dict, f"best_vgn_{self.net_name}_val_acc={score:.4f}.pt", f"best_vgn_{self.net_name}_val_acc=*.pt")

    def save_state(self, state):
        return self._write(state, "trainer_state.pt")

    def load_for_resume(self):
        """(state dict of the newest epoch file, trainer state); ValueError when either is missing or the two are not of one
        iteration (a run that was killed between the two writes)"""
        files = self.epoch_files()
        if not files or not os.path.exists(self.state_path):
            raise ValueError(f"{self.dir} holds no vgn_{self.net_name}_*.pt with its trainer_state.pt to resume from")
        iteration, path = files[-1]
        saved = torch.load(self.state_path, map_location="cpu")
        if int(saved["iteration"]) != iteration:
            raise ValueError(f"{path} is of iteration {iteration}, trainer_state.pt of iteration {int(saved['iteration'])}: "
                             "the two were not written by one epoch")
        return torch.load(path, map_location="cpu"), saved


def sync_parameters_(net, group=None):
    """Make the replicas of a data-parallel run equal: flatten the parameters and broadcast rank 0's over `group`, in place
    -> [flat parameter].  Every rank builds its own network (torch's random initialisation, or a file only rank 0 may have), and
    averaged gradients keep replicas equal only if they start equal.  Without an initialised process group only the flattening."""
    import torch.distributed as dist
    flat = net.flatten_parameters()
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        with torch.no_grad():
            dist.broadcast(flat[0].data, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return flat


def common_steps(batches, group=None, device=None):
    """How many batches of `batches` every rank of `group` runs per epoch: the smallest `len()` over the ranks, because each step
    and each epoch end is a collective that every rank must enter equally often (`ResidentBatches` gives the ranks shares that
    differ by one row, and `drop_last` is applied per rank).  None without a group or without batches."""
    import torch.distributed as dist
    if batches is None or group is None or not (dist.is_available() and dist.is_initialized()):
        return None
    if not hasattr(batches, "__len__"):
        raise TypeError("under a process group the batches need a len(): the ranks agree on the steps of an epoch beforehand")
    n = torch.tensor([len(batches)], dtype=torch.int64, device=device)
    dist.all_reduce(n, op=dist.ReduceOp.MIN, group=group)
    return int(n.item())


def _line(name, metrics):
    return name + "".join(f" {k}: {v:.4f}" for k, v in metrics.items())          # train_giga.py:76-79


class Trainer:
    """`create_trainer` + `create_evaluator` + the handlers of train_giga.py:62-120.  `train_batches` / `val_batches`: iterables
    of `(x, pos, pos_occ, y)` on the device of `net` (`ResidentBatches`), one pass = one epoch.  `on_step(trainer, batch, out,
    loss_dict)` sees each step's own tensors (`trainer.phase` is "train" or "val"; `out` is the 4-tuple the loss took).  With a
    `group`, every rank runs its own batches, the flat gradient is averaged over the group each step and the metrics are summed
    over it each epoch; rank 0 writes the files.  The constructor then broadcasts rank 0's parameters (`sync_parameters_`) and
    fixes the steps of an epoch and of a validation pass to the smallest count over the ranks (`common_steps`), so that every rank
    enters every collective; all ranks skip a validation pass that has no batch on one of them.  `quiet=True` drops the
    `Train …` / `Val …` lines (the reference's `--silence` hides its progress bar, which does not exist here)."""

    finalize = staticmethod(finalize_metrics)                # the accumulator words of an epoch -> its metrics
    score_key = "accuracy"                                   # the validation metric that names the "best" file (train_giga.py:93-95)

    @staticmethod
    def _check_net(net_name):
        if net_name == "giga_geo":
            raise NotImplementedError("giga_geo has no quality head, hence none of these epoch metrics; GeoTrainer runs it")
        if net_name not in NETS:
            raise ValueError(f"net_name is one of {NETS}")

    def __init__(self, net, train_batches, val_batches=None, lr=2e-4, net_name="giga", logdir=None, precision=None, group=None,
                 resume=False, on_step=None, quiet=False):
        net_name = str(net_name).lower()
        self._check_net(net_name)
        self.net, self.net_name, self.train_batches, self.val_batches = net, net_name, train_batches, val_batches
        self.group, self.on_step, self.quiet, self.phase = group, on_step, bool(quiet), None
        if precision is not None:
            net.set_train_precision(precision)
        self.rank = 0
        if group is not None:
            import torch.distributed as dist
            self.rank = dist.get_rank(group)
        # every rank reads the directory (resume); only rank 0 writes to it and checks that a new run starts in an empty one
        self.ckpt = Checkpoints(logdir, net_name, resume or self.rank != 0) if logdir is not None else None
        self.logdir = str(logdir) if logdir is not None else None
        self.epoch, self.iteration = 0, 0
        saved = None
        if resume:
            if self.ckpt is None:
                raise ValueError("resume=True continues the run of a logdir")
            state_dict, saved = self.ckpt.load_for_resume()
            net.load_state_dict(state_dict)
        flat = sync_parameters_(net, group)                  # (after the resume load: the ranks start from rank 0's weights)
        _capi.require_device(flat[0])
        self.device = flat[0].device
        self.optimizer = FlatAdam(flat, lr=lr)
        self.metrics, self.val_metrics = TrainMetrics(self.device), TrainMetrics(self.device)
        self.train_steps = common_steps(train_batches, group, self.device)
        self.val_steps = common_steps(val_batches, group, self.device)
        if saved is not None:
            self.optimizer.load_state_dict(saved["optimizer"])
            self.epoch, self.iteration = int(saved["epoch"]), int(saved["iteration"])
            self.ckpt.best_score = saved["best_score"]
            for batches, key in ((train_batches, "train_batches"), (val_batches, "val_batches")):
                if batches is not None and saved.get(key) is not None:
                    batches.seed, batches.epoch = saved[key]["seed"], saved[key]["epoch"]

    @property
    def best_score(self):
        return self.ckpt.best_score if self.ckpt is not None else None

    def _forward(self, batch, metrics):
        x, pos, pos_occ, y = batch
        if self.net_name == "giga_aff":                      # no occupancy head: the same loss kernels with M = 0
            qual, rot, width = self.net(x, pos)
            out = (qual, rot, width, qual.new_empty((qual.shape[0], 0)))
            y = (y[0], y[1], y[2], y[3][:, :0])
        else:
            out = self.net(x, pos, p_tsdf=pos_occ)
        loss, loss_dict = giga_loss(out, y, metrics=metrics)
        return out, loss, loss_dict

    def train_step(self, batch):
        """one optimisation step (train_giga.py:199-211); nothing here reads a device value on the host"""
        self.optimizer.zero_grad(set_to_none=True)
        out, loss, loss_dict = self._forward(batch, self.metrics)
        loss.backward()
        if self.group is not None:
            allreduce_mean_(self.optimizer.param_groups[0]["params"][0].grad, self.group)
        self.optimizer.step()
        self.iteration += 1
        if self.on_step is not None:
            self.on_step(self, batch, out, loss_dict)
        return loss

    def train_epoch(self):
        """one pass over `train_batches` -> the epoch's metrics (METRIC_KEYS)"""
        self.net.train()
        self.metrics.reset()
        self.phase = "train"
        for batch in itertools.islice(self.train_batches, self.train_steps):     # (None: all of them)
            self.train_step(batch)
        self.phase = None
        self.epoch += 1
        return self.finalize(self.metrics.all_reduce(self.group).words())

    def validate(self):
        """`create_evaluator` (train_giga.py:221-235) over `val_batches` -> the metrics, or None without a validation batch"""
        if self.val_batches is None or self.val_steps == 0:  # (0: some rank has no batch, so no rank enters the reduction)
            return None
        self.net.eval()
        self.val_metrics.reset()
        self.phase, n = "val", 0
        try:
            with torch.no_grad():
                for batch in itertools.islice(self.val_batches, self.val_steps):
                    out, _, loss_dict = self._forward(batch, self.val_metrics)
                    n += 1
                    if self.on_step is not None:
                        self.on_step(self, batch, out, loss_dict)
        finally:
            self.phase = None
            self.net.train()
        if n == 0 and self.val_steps is None:                # (drop_last=True on a small validation set; one rank, no collective)
            return None
        return self.finalize(self.val_metrics.all_reduce(self.group).words())

    def state(self):
        """what `resume=True` needs beside the network's own file"""
        def of(batches):
            return {"seed": int(batches.seed), "epoch": int(batches.epoch)} if hasattr(batches, "seed") and hasattr(batches, "epoch") else None
        return {"optimizer": self.optimizer.state_dict(), "epoch": self.epoch, "iteration": self.iteration,
                "best_score": self.best_score, "train_batches": of(self.train_batches), "val_batches": of(self.val_batches)}

    def run(self, max_epochs):
        """epochs `self.epoch + 1 .. max_epochs`: train, validate, log, checkpoint -> the list of per-epoch records"""
        records = []
        while self.epoch < int(max_epochs):
            train = self.train_epoch()
            val = self.validate()
            record = {"epoch": self.epoch, "iteration": self.iteration, "train": train, "val": val}
            records.append(record)
            if self.rank != 0:
                continue
            if not self.quiet:
                print(_line("Train", train))
                if val is not None:
                    print(_line("Val", val))
            if self.ckpt is not None:
                # each file is written whole or not at all; a run killed between the epoch file and the trainer state leaves a
                # pair of two iterations, which resume=True refuses
                sd = self.net.state_dict()
                if val is not None:
                    self.ckpt.save_best(sd, val[self.score_key])
                self.ckpt.save_epoch(sd, self.iteration)
                self.ckpt.save_state(self.state())
                with open(os.path.join(self.logdir, "metrics.jsonl"), "a") as f:
                    f.write(json.dumps(record) + "\n")
        return records


class GeoTrainer(Trainer):
    """`create_trainer` + `create_evaluator` + the handlers of the reference's scripts/train_giga_geo.py:59-118 for the
    occupancy-only model `giga_geo`, on `Trainer`'s machinery: the same `(x, pos, pos_occ, y)` batches (the script trains on the
    grasp rows of `DatasetVoxelOccFile` and ignores their grasp fields: `pos` and `y[:3]` are not read), `FlatAdam`, `group`,
    `resume`, checkpoints, `metrics.jsonl` and `quiet`.  A step is `net(x, None, p_tsdf=pos_occ)`, `geo_loss` and its backward; the
    epoch metrics are GEO_METRIC_KEYS, counted over every occupancy point by the loss launch (`finalize_geo_metrics`); the files are
    `vgn_giga_geo_<iteration>.pt` and `best_vgn_giga_geo_val_acc=<occ_accuracy>.pt` (train_giga_geo.py:91-93).
    `on_step(trainer, batch, out, loss_dict)` gets `out = (None, None, None, logits)`, the shape of the script's `select`, and
    `loss_dict = {"loss": ...}`."""

    finalize = staticmethod(finalize_geo_metrics)
    score_key = "occ_accuracy"

    @staticmethod
    def _check_net(net_name):
        if net_name != "giga_geo":
            raise ValueError(f"GeoTrainer runs giga_geo; Trainer runs {NETS}")

    def __init__(self, net, train_batches, val_batches=None, lr=2e-4, net_name="giga_geo", **kwargs):
        super().__init__(net, train_batches, val_batches, lr=lr, net_name=net_name, **kwargs)

    def _forward(self, batch, metrics):
        x, _, pos_occ, y = batch
        logits = self.net(x, None, p_tsdf=pos_occ)
        loss, loss_dict = geo_loss(logits, y[3], metrics=metrics)
        return (None, None, None, logits), loss, loss_dict
