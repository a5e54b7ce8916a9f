"""CPU tests of the training loop's host side (giga_amd.trainer, giga_amd.train): the metrics from the accumulator words, the
train / validation split, the argument checks of giga_train_loss_metrics, the checkpoint files, the command line and the
reduction of the accumulator over two gloo ranks."""
import ctypes
import os
import re
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import trainer_emu as E
from giga_amd import _capi, networks, train, trainer, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_words(sums=(0.0,) * 5, **counts):
    w = np.zeros(E.WORDS, np.uint64)
    for k, v in counts.items():
        w[E.COUNTS.index(k)] = v
    w.view(np.float64)[E.SUM_WORD:E.SUM_WORD + 5] = sums
    return w


# ------------------------------------------------------------------------------------------------------------ metrics
def test_finalize_metrics_ordinary_words():
    assert trainer.WORDS == E.WORDS and trainer.COUNT_NAMES == E.COUNTS and trainer.SUM_WORD == E.SUM_WORD
    assert trainer.METRIC_KEYS == E.KEYS and tuple(trainer.LOSS_KEYS) == E.LOSS_ORDER
    w = make_words(batches=3, examples=96, correct=70, tp=30, fp=11, fn=15, sums=(1.5, 0.75, 0.1, 2.25, 4.0))
    w[7] = w[13] = w[15] = 0xDEADBEEF                        # reserved words do not matter
    m = trainer.finalize_metrics(w)
    assert list(m) == list(E.KEYS) and all(type(v) is float for v in m.values())
    assert m["accuracy"] == 70 / 96 and m["precision"] == 30 / (41 + 1e-20) and m["recall"] == 30 / (45 + 1e-20)
    assert [m[k] for k in E.LOSS_ORDER] == [1.5 / 3, 0.75 / 3, 0.1 / 3, 2.25 / 3, 4.0 / 3]
    assert m == E.finalize(w)
    assert trainer.finalize_metrics(w.view(np.int64)) == m   # the words as the device tensor holds them
    with pytest.raises(ValueError):
        trainer.finalize_metrics(w[:15])


def test_finalize_metrics_without_positives():
    m = trainer.finalize_metrics(make_words(batches=2, examples=8, correct=5, tp=0, fp=0, fn=3))
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["accuracy"] == 5 / 8          # no predicted positives
    m = trainer.finalize_metrics(make_words(batches=2, examples=8, correct=8, tp=0, fp=0, fn=0))
    assert m["precision"] == 0.0 and m["recall"] == 0.0 and m["accuracy"] == 1.0            # no positives at all


def test_finalize_metrics_raises():
    with pytest.raises(ValueError, match="batch"):
        trainer.finalize_metrics(make_words())
    with pytest.raises(ValueError, match="3 scenes"):
        trainer.finalize_metrics(make_words(batches=1, examples=5, correct=5, invalid=3))


def test_emulated_update():
    """the restatement itself, on a hand-counted batch"""
    half = np.float32(0.5)
    q = np.array([0.0, 1.0, half, np.nextafter(half, np.float32(1)), np.nextafter(half, np.float32(0)), 0.9, np.nan, 1.5, 0.2], np.float32)
    y = np.array([0, 1, 1, 0, 0, 1, 1, 0, 0.3], np.float32)
    w = make_words()
    w[7], w[14] = 77, 99
    w = E.update(w, q, y, np.arange(5, dtype=np.float32))
    # valid: the first six.  pred: 0 1 0 1 0 1; label: 0 1 1 0 0 1
    assert w[:7].tolist() == [1, 6, 4, 2, 1, 1, 3] and w[7] == 77 and w[14] == 99
    assert w.view(np.float64)[8:13].tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    w = E.update(w, q[:1], y[:1], np.full(5, 0.1, np.float32))
    assert w[:7].tolist() == [2, 7, 5, 2, 1, 1, 3]
    assert w.view(np.float64)[12] == 4.0 + np.float64(np.float32(0.1))


# -------------------------------------------------------------------------------------------------------------- split
@pytest.mark.parametrize("n,val_split,val_size", [(30, 0.1, 3), (30, 0.2, 6), (7, 0.1, 0), (1000, 0.1, 100), (33, 0.5, 16), (10, 0.0, 0),
                                                  (29, 0.1, 2)])
def test_train_val_split(n, val_split, val_size):
    tr, va = trainer.train_val_split(n, val_split, seed=4)
    assert val_size == int(val_split * n)                    # create_train_val_loaders' sizes
    assert len(va) == val_size and len(tr) == n - val_size and tr.dtype == va.dtype == np.int64
    assert sorted(np.concatenate([tr, va]).tolist()) == list(range(n))
    order = np.random.default_rng([4, 0]).permutation(n)
    assert np.array_equal(tr, order[:n - val_size]) and np.array_equal(va, order[n - val_size:])
    again = trainer.train_val_split(n, val_split, seed=4)
    assert np.array_equal(again[0], tr) and np.array_equal(again[1], va)
    if n >= 29:
        other = trainer.train_val_split(n, val_split, seed=5)
        assert not np.array_equal(other[0], tr)


# -------------------------------------------------------------------------------------------------------------- C ABI
P = 0x10000000                            # never dereferenced: every check precedes the first HIP call


def test_metrics_entry_argument_checks_without_a_gpu():
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    name = "giga_train_loss_metrics"
    assert hasattr(L, name) and name in _capi.EXPORTS and L.giga_abi_version() == 3
    decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert decl is not None
    params = [p.strip() for p in decl.group(1).split(",")]
    res, args = _capi._SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == len(params) == 14
    for p, a in zip(params, args):                           # pointers are void pointers in the table, the two sizes ints
        assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int), p
    assert params[8:10] == ["int B", "int M"] and params[12] == "void* acc"
    assert "#define GIGA_TRAIN_METRICS_BYTES %d\n" % _capi.TRAIN_METRICS_BYTES in hdr and _capi.TRAIN_METRICS_BYTES == 8 * E.WORDS

    def call(B=2, M=8, ins=(P,) * 8, losses=P, scene=P, acc=P):
        return getattr(L, name)(*ins, B, M, losses, scene, acc, None)

    assert call(acc=None) == -1 and call(acc=None, B=0) == -1
    for off in (1, 2, 4, 7, 12):
        assert call(acc=P + off) == -1 and call(acc=P + off, B=0) == -1
    assert call(B=-1) == -1 and call(M=-1) == -1
    assert call(B=0) == 0 and call(B=0, M=0) == 0
    assert call(acc=P + 8, B=0) == 0                         # 8-byte alignment is all it asks
    for i in (0, 1, 2, 4, 5, 6):                             # the checks of giga_train_loss
        assert call(ins=tuple(None if j == i else P for j in range(8))) == -1
    for i in (3, 7):                                         # occupancy logits and targets: read only when M > 0
        assert call(ins=tuple(None if j == i else P for j in range(8))) == -1
    assert call(losses=None) == -1 and call(scene=None) == -1


# -------------------------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_files(tmp_path):
    net = networks.get_network("giga")                       # a CPU module: only its state dict is written
    net.load_state_dict(weights.make_state_dict(3))
    sd = net.state_dict()
    logdir = tmp_path / "run"
    ck = trainer.Checkpoints(logdir, "giga")
    names = lambda: sorted(p.name for p in logdir.iterdir())  # noqa: E731
    first = ck.save_epoch(sd, 7)
    assert names() == ["vgn_giga_7.pt"] and first == str(logdir / "vgn_giga_7.pt")
    got = torch.load(first)
    shapes = weights.giga_param_shapes()
    assert list(got) == list(shapes) == list(sd)
    assert all(tuple(got[k].shape) == tuple(shapes[k]) and torch.equal(got[k], sd[k]) for k in shapes)
    loaded = networks.load_network(first, "cpu")             # the model name from the file stem, as the reference's loader
    assert all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), sd.values()))
    ck.save_epoch(sd, 14)
    assert names() == ["vgn_giga_14.pt"]                     # one at a time
    ck.save_epoch(sd, 105)
    assert names() == ["vgn_giga_105.pt"] and ck.epoch_files() == [(105, str(logdir / "vgn_giga_105.pt"))]
    # "best": only on a strictly greater score
    assert ck.best_score is None
    assert ck.save_best(sd, 0.5) == str(logdir / "best_vgn_giga_val_acc=0.5000.pt")
    assert ck.save_best(sd, 0.5) is None and ck.save_best(sd, 0.25) is None and ck.best_score == 0.5
    assert names() == ["best_vgn_giga_val_acc=0.5000.pt", "vgn_giga_105.pt"]
    assert ck.save_best(sd, 0.62505) is not None and ck.best_score == 0.62505
    assert names() == ["best_vgn_giga_val_acc=0.6250.pt", "vgn_giga_105.pt"]
    assert list(torch.load(logdir / "best_vgn_giga_val_acc=0.6250.pt")) == list(shapes)
    # a directory that holds checkpoints is refused (require_empty=True) unless the run is resumed
    with pytest.raises(ValueError, match="resume"):
        trainer.Checkpoints(logdir, "giga")
    resumed = trainer.Checkpoints(logdir, "giga", resume=True)
    assert resumed.epoch_files() == [(105, str(logdir / "vgn_giga_105.pt"))]
    # resuming pairs the newest epoch file with a trainer state of the same iteration, and refuses any other pair
    with pytest.raises(ValueError, match="trainer_state"):
        resumed.load_for_resume()
    assert resumed.save_state({"iteration": 105, "epoch": 15}) == resumed.state_path == str(logdir / "trainer_state.pt")
    got_sd, state = resumed.load_for_resume()
    assert state == {"iteration": 105, "epoch": 15} and list(got_sd) == list(shapes)
    resumed.save_epoch(sd, 112)                              # a run killed before the state of iteration 112 was written
    with pytest.raises(ValueError, match="iteration 112.*iteration 105"):
        resumed.load_for_resume()
    resumed.save_state({"iteration": 112, "epoch": 16})
    assert resumed.load_for_resume()[1]["epoch"] == 16
    assert not [n for n in names() if n.endswith(".tmp")]    # every file is written under another name and moved into place
    (tmp_path / "notes").mkdir()
    (tmp_path / "notes" / "readme.txt").write_text("no checkpoints here")
    trainer.Checkpoints(tmp_path / "notes", "giga")          # other files do not count
    # the other models' names
    aff = networks.get_network("giga_aff")
    path = trainer.Checkpoints(tmp_path / "aff", "giga_aff").save_epoch(aff.state_dict(), 3)
    assert os.path.basename(path) == "vgn_giga_aff_3.pt" and list(torch.load(path)) == list(weights.giga_param_shapes(with_tsdf=False))
    assert Path(path).stem.split("_")[1:-1] == ["giga", "aff"]


def test_trainer_refuses_giga_geo():
    with pytest.raises(NotImplementedError):
        trainer.Trainer(None, [], net_name="giga_geo")
    with pytest.raises(ValueError):
        trainer.Trainer(None, [], net_name="vgn")
    with pytest.raises(_capi.GigaHipError):
        trainer.TrainMetrics("cpu")
    import giga_amd
    assert giga_amd.Trainer is trainer.Trainer and giga_amd.TrainMetrics is trainer.TrainMetrics
    assert giga_amd.train_val_split is trainer.train_val_split


# -------------------------------------------------------------------------------------------------------- command line
def test_parser_accepts_the_reference_command_line():
    parser = train.build_parser()
    a = parser.parse_args(["--dataset", "data/set", "--dataset_raw", "data/set_raw"])
    assert (a.net, a.epochs, a.batch_size, a.lr, a.val_split) == ("giga", 10, 32, 2e-4, 0.1)
    assert (a.augment, a.silence, a.load_path, a.description, a.savedir) == (False, False, "", "", "")
    assert a.dataset == Path("data/set") and a.dataset_raw == Path("data/set_raw") and Path(a.logdir) == Path("data/runs")
    assert (a.precision, a.seed, a.resume) == ("fp32", 0, False)
    b = parser.parse_args("--net giga_aff --dataset d --dataset_raw r --logdir runs --description try --savedir out --epochs 3 "
                          "--batch-size 16 --lr 1e-3 --val-split 0.2 --augment --silence --load-path w.pt --precision bf16 --seed 9 "
                          "--resume".split())
    assert (b.net, b.epochs, b.batch_size, b.lr, b.val_split, b.augment, b.silence) == ("giga_aff", 3, 16, 1e-3, 0.2, True, True)
    assert (b.load_path, b.precision, b.seed, b.resume, b.savedir) == ("w.pt", "bf16", 9, True, "out")
    with pytest.raises(SystemExit):
        parser.parse_args(["--dataset", "d"])                # --dataset_raw is required
    with pytest.raises(SystemExit):
        parser.parse_args(["--dataset", "d", "--dataset_raw", "r", "--precision", "fp8"])
    # --resume names its directory: a generated name carries the time of this start
    with pytest.raises(SystemExit):
        train.parse_args(["--dataset", "d", "--dataset_raw", "r", "--resume"])
    assert train.parse_args(["--dataset", "d", "--dataset_raw", "r", "--resume", "--savedir", "out"]).resume is True
    assert train.parse_args(["--dataset", "d", "--dataset_raw", "r"]).resume is False
    from datetime import datetime
    assert train.run_directory(b) == Path("out")
    a.description = "note"
    assert train.run_directory(a, datetime(2024, 3, 5, 14, 7)) == \
        Path("data/runs") / "24-03-05-14-07_dataset=set,augment=False,net=giga,batch_size=32,lr=2e-04,note"
    a.description = ""
    assert train.run_directory(a, datetime(2024, 3, 5, 14, 7)).name == "24-03-05-14-07_dataset=set,augment=False,net=giga,batch_size=32,lr=2e-04"


# -------------------------------------------------------------------------------------------------------------- gloo
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_words(rank):
    w = make_words(batches=3 + rank, examples=90 + 7 * rank, correct=50 + rank, tp=20, fp=3 * rank, fn=4, invalid=0,
                   sums=(0.1 * (rank + 1), 0.25, 1e-3 * (rank + 2), 3.0, 7.5 + rank))
    w[7], w[13], w[15] = 11 + rank, 12 + rank, 13 + rank
    return w


def _reduce_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    acc = torch.from_numpy(_rank_words(rank).view(np.int64).copy())
    trainer.all_reduce_words_(acc)
    np.save(os.path.join(out_dir, f"w{rank}.npy"), acc.numpy())
    dist.barrier()
    dist.destroy_process_group()


class _Share:
    """a rank's batches, as far as `common_steps` looks at them"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def _replica_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.manual_seed(100 + rank)                            # every rank draws its own initialisation, as under torchrun
    net = networks.get_network("giga")
    before = torch.cat([p.detach().reshape(-1) for p in net._ordered_params()]).clone()
    flat = trainer.sync_parameters_(net, dist.group.WORLD)
    assert flat[0] is net.flatten_parameters()[0] and flat[0].requires_grad
    # 127 rows over two ranks at batch 32, drop_last per rank: 64 rows -> 2 batches, 63 rows -> 1; and a validation share of 1 | 0
    from giga_amd.resident import batch_bounds
    mine = len(range(rank, 127, world))
    steps = trainer.common_steps(_Share(len(batch_bounds(mine, 32, True))), dist.group.WORLD)
    val_steps = trainer.common_steps(_Share(1 - rank), dist.group.WORLD)
    with pytest.raises(TypeError):                           # batches without a len() cannot be agreed on beforehand
        trainer.common_steps(iter([]), dist.group.WORLD)
    # the Trainer's loop shape on those counts: one collective per step, one at the end; it ends on both ranks
    import itertools
    done = 0
    for _ in itertools.islice(range(len(batch_bounds(mine, 32, True))), steps):
        g = torch.full((4,), float(rank + 1))
        trainer.allreduce_mean_(g, dist.group.WORLD)
        done += int(g[0].item() == 1.5)
    acc = torch.zeros(16, dtype=torch.int64)
    acc[0] = done
    trainer.all_reduce_words_(acc, dist.group.WORLD)
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), before=before.numpy(), after=flat[0].detach().numpy(),
             state=torch.cat([v.reshape(-1) for v in net.state_dict().values()]).numpy(),
             counts=np.array([mine, steps, val_steps, done, int(acc[0])]), none=np.array(trainer.common_steps(None, dist.group.WORLD) is None))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_replicas_start_equal_and_run_equal_steps_gloo(tmp_path):
    port = _free_port()
    mp.spawn(_replica_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(tmp_path, f"r{r}.npz")) for r in range(2))
    assert not np.array_equal(r0["before"], r1["before"])                        # they did start apart
    for r in (r0, r1):
        assert np.array_equal(r["after"].view(np.uint32), r0["before"].view(np.uint32))          # rank 0's bytes on every rank
        assert np.array_equal(r["state"].view(np.uint32), r0["before"].view(np.uint32))          # ... and in the named views
        assert bool(r["none"])
    assert r0["counts"].tolist() == [64, 1, 0, 1, 2] and r1["counts"].tolist() == [63, 1, 0, 1, 2]
    # one process, no group: the batches' own length decides (None), and nothing is broadcast
    net = networks.get_network("giga")
    assert trainer.common_steps(_Share(3)) is None and trainer.sync_parameters_(net)[0] is net.flatten_parameters()[0]


@pytest.mark.timeout(300)
def test_accumulator_all_reduce_gloo(tmp_path):
    port = _free_port()
    mp.spawn(_reduce_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    w0, w1 = _rank_words(0), _rank_words(1)
    for r, mine in enumerate((w0, w1)):
        got = np.load(os.path.join(tmp_path, f"w{r}.npy")).view(np.uint64)
        assert got[:7].tolist() == (w0[:7] + w1[:7]).tolist()
        assert np.array_equal(got.view(np.float64)[8:13], w0.view(np.float64)[8:13] + w1.view(np.float64)[8:13])
        assert got[[7, 13, 14, 15]].tolist() == mine[[7, 13, 14, 15]].tolist()       # reserved words stay the rank's own
    m = trainer.finalize_metrics(np.load(os.path.join(tmp_path, "w0.npy")))
    assert m["accuracy"] == 101 / 187 and m["loss_all"] == (7.5 + 8.5) / 7
    # without an initialised process group the reduction leaves the words alone
    acc = torch.from_numpy(w0.view(np.int64).copy())
    assert np.array_equal(trainer.all_reduce_words_(acc).numpy().view(np.uint64), w0)
