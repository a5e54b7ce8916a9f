"""CPU tests of the giga_geo training loop's host side (giga_amd.trainer.GeoTrainer, giga_amd.train_geo): the metrics from the
accumulator words, the numpy restatement of the accumulator, the argument checks of the three giga_train_occ_loss entry points, the
checkpoint files and the command line."""
import ctypes
import os
import re
from datetime import datetime
from pathlib import Path

import numpy as np
import pytest
import torch

import geo_trainer_emu as G
from giga_amd import _capi, networks, train, train_geo, trainer, weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_words(loss_sum=0.0, **counts):
    w = np.zeros(G.WORDS, np.uint64)
    for k, v in counts.items():
        w[G.COUNTS.index(k)] = v
    for k in G.LOSS_WORDS:
        w.view(np.float64)[k] = loss_sum
    return w


# ------------------------------------------------------------------------------------------------------------ metrics
def test_finalize_geo_metrics_ordinary_words():
    assert trainer.GEO_METRIC_KEYS == G.KEYS == ("loss", "occ_accuracy", "occ_precision", "occ_recall")
    assert trainer.WORDS == G.WORDS and trainer.COUNT_NAMES == G.COUNTS and trainer.SUM_WORD == G.SUM_WORD
    assert tuple(trainer.SUM_WORD + trainer.LOSS_KEYS.index(k) for k in ("loss_occ", "loss_all")) == G.LOSS_WORDS
    w = make_words(batches=3, examples=3 * 4 * 64, correct=500, tp=130, fp=41, fn=75, loss_sum=2.25)
    w[7] = w[13] = w[15] = 0xDEADBEEF                        # reserved words do not matter
    w.view(np.float64)[8:11] = (7.0, -3.0, 1e9)              # nor do the sums the occupancy loss leaves alone
    m = trainer.finalize_geo_metrics(w)
    assert list(m) == list(G.KEYS) and all(type(v) is float for v in m.values())
    assert m["occ_accuracy"] == 500 / 768 and m["occ_precision"] == 130 / (171 + 1e-20) and m["occ_recall"] == 130 / (205 + 1e-20)
    assert m["loss"] == 2.25 / 3
    assert m == G.finalize(w)
    assert trainer.finalize_geo_metrics(w.view(np.int64)) == m          # the words as the device tensor holds them
    # the same words through the grasp trainer's finalize: the same counts, and the loss under both of its names
    old = trainer.finalize_metrics(w)
    assert (old["accuracy"], old["precision"], old["recall"]) == (m["occ_accuracy"], m["occ_precision"], m["occ_recall"])
    assert m["loss"] == old["loss_occ"] == old["loss_all"]
    with pytest.raises(ValueError):
        trainer.finalize_geo_metrics(w[:15])
    with pytest.raises(ValueError):
        trainer.finalize_geo_metrics(w.astype(np.uint32))


def test_finalize_geo_metrics_without_positives():
    for w in (make_words(batches=2, examples=512, correct=400, tp=0, fp=0, fn=112, loss_sum=1.0),     # none predicted
              make_words(batches=2, examples=512, correct=512, tp=0, fp=0, fn=0, loss_sum=0.5),       # no positives at all
              make_words(batches=1, examples=64, correct=60, tp=0, fp=4, fn=0, loss_sum=0.5)):        # no positive target
        m, old = trainer.finalize_geo_metrics(w), trainer.finalize_metrics(w)
        assert m["occ_precision"] == 0.0 and m["occ_recall"] == 0.0
        assert m["occ_accuracy"] == int(w[2]) / int(w[1]) and m == G.finalize(w)
        assert (old["accuracy"], old["precision"], old["recall"]) == (m["occ_accuracy"], m["occ_precision"], m["occ_recall"])
        assert m["loss"] == old["loss_occ"] == old["loss_all"]


def test_finalize_geo_metrics_raises():
    with pytest.raises(ValueError, match="batch"):
        trainer.finalize_geo_metrics(make_words())
    with pytest.raises(ValueError, match="3 points"):
        trainer.finalize_geo_metrics(make_words(batches=1, examples=61, correct=5, invalid=3))
    with pytest.raises(ValueError, match="batch"):           # finalize_metrics raises at the same two places
        trainer.finalize_metrics(make_words())
    with pytest.raises(ValueError, match="3 scenes"):
        trainer.finalize_metrics(make_words(batches=1, examples=61, correct=5, invalid=3))


def test_emulated_update():
    """the restatement itself, on a hand-counted batch"""
    inf = np.inf
    z = np.array([[0.0, -0.0, 1e-6, -1e-6, 120.0], [-120.0, inf, -inf, np.nan, 2.0], [1.0, -1.0, 3.0, -3.0, 0.5]], np.float32)
    t = np.array([[1, 0, 1, 1, 0], [0, 1, 1, 1, 0.5], [2, 0, 1, 0, 1]], np.float32)
    # pred:          0  0  1  0  1     0  1  0  -  1       1  0  1  0  1
    # valid:         y  y  y  y  y     y  y  y  n  n       n  y  y  y  y        (NaN logit; targets 0.5 and 2)
    # correct:       n  y  y  n  n     y  y  n             .  y  y  y  y
    w = make_words()
    w[7], w[14] = 77, 99
    w.view(np.float64)[8:11] = (1.5, 2.5, 3.5)
    w = G.update(w, z, t, np.float32(0.7))
    assert w[:7].tolist() == [1, 12, 8, 4, 1, 3, 3] and w[7] == 77 and w[14] == 99
    assert w.view(np.float64)[8:13].tolist() == [1.5, 2.5, 3.5, np.float64(np.float32(0.7)), np.float64(np.float32(0.7))]
    w = G.update(w, z[2:, 1:], t[2:, 1:], np.float32(0.1))
    assert w[:7].tolist() == [2, 16, 12, 6, 1, 3, 3]
    assert w.view(np.float64)[11] == w.view(np.float64)[12] == np.float64(np.float32(0.7)) + np.float64(np.float32(0.1))
    with pytest.raises(AssertionError):                      # the band where the last bit of exp decides is not emulated
        G.update(w, np.float32([[1e-9]]), np.float32([[1]]), 0.0)
    rng = np.random.default_rng(5)
    e = G.edge_logits((3, 7), rng)
    assert set(np.float32([0.0, 1e-6, -1e-6, 120, -120, inf, -inf]).tolist()) <= set(e.reshape(-1).tolist())
    assert np.signbit(e[e == 0]).any() and not np.signbit(e[e == 0]).all()
    assert G.edge_logits((1, 1), rng).shape == (1, 1)


# -------------------------------------------------------------------------------------------------------------- C ABI
P = 0x10000000                            # never dereferenced: every check precedes the first HIP call
NAMES = ("giga_train_occ_loss", "giga_train_occ_loss_metrics", "giga_train_occ_loss_backward")


def test_occ_loss_entries_are_declared_and_exported():
    L = _capi.lib()
    hdr = open(os.path.join(ROOT, "include", "giga_hip.h")).read()
    assert L.giga_abi_version() == 3
    want = {"giga_train_occ_loss": ["const float* occ_logits", "const float* occ_target", "int B", "int M", "float* loss",
                                    "float* scene_losses", "void* stream"],
            "giga_train_occ_loss_metrics": ["const float* occ_logits", "const float* occ_target", "int B", "int M", "float* loss",
                                            "float* scene_losses", "uint32_t* scene_counts", "void* acc", "void* stream"],
            "giga_train_occ_loss_backward": ["const float* occ_logits", "const float* occ_target", "const float* grad_loss", "int B",
                                             "int M", "float* docc", "void* stream"]}
    for name in NAMES:
        assert hasattr(L, name) and name in _capi.EXPORTS
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert decl is not None
        params = [" ".join(p.split()) for p in decl.group(1).split(",")]
        assert params == want[name]
        res, args = _capi._SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(params)
        for p, a in zip(params, args):                       # pointers are void pointers in the table, the two sizes ints
            assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int), p
    assert "#define GIGA_TRAIN_METRICS_BYTES %d\n" % _capi.TRAIN_METRICS_BYTES in hdr and _capi.TRAIN_METRICS_BYTES == 8 * G.WORDS


def test_occ_loss_argument_checks_without_a_gpu():
    L = _capi.lib()

    def plain(B=2, M=8, z=P, t=P, loss=P, scene=P):
        return L.giga_train_occ_loss(z, t, B, M, loss, scene, None)

    def metrics(B=2, M=8, z=P, t=P, loss=P, scene=P, counts=P, acc=P):
        return L.giga_train_occ_loss_metrics(z, t, B, M, loss, scene, counts, acc, None)

    def backward(B=2, M=8, z=P, t=P, g=P, docc=P):
        return L.giga_train_occ_loss_backward(z, t, g, B, M, docc, None)

    for call in (plain, metrics, backward):
        assert call(B=-1) == -1 and call(M=-1) == -1 and call(B=-1, M=0) == -1
        assert call(M=0) == -1 and call(B=1, M=0) == -1      # an empty mean
        assert call(B=0) == 0 and call(B=0, M=0) == 0        # an empty batch: nothing to do
        assert call(z=None) == -1 and call(t=None) == -1
    assert plain(loss=None) == -1 and plain(scene=None) == -1
    assert metrics(loss=None) == -1 and metrics(scene=None) == -1 and metrics(counts=None) == -1
    assert backward(g=None) == -1 and backward(docc=None) == -1
    assert metrics(acc=None) == -1 and metrics(acc=None, B=0) == -1
    for off in (1, 2, 4, 7, 12):
        assert metrics(acc=P + off) == -1 and metrics(acc=P + off, B=0) == -1
    assert metrics(acc=P + 8, B=0) == 0                      # 8-byte alignment is all it asks
    # B == 0 leaves the accumulator alone: real host memory, which a launch could not even address
    acc = np.arange(100, 116, dtype=np.uint64)
    before = acc.copy()
    assert metrics(B=0, acc=acc.ctypes.data) == 0 and metrics(B=0, M=0, acc=acc.ctypes.data) == 0
    assert np.array_equal(acc, before)


# -------------------------------------------------------------------------------------------------------- the classes
def test_trainers_divide_the_nets():
    with pytest.raises(NotImplementedError, match="GeoTrainer"):
        trainer.Trainer(None, [], net_name="giga_geo")
    for name in trainer.NETS + ("vgn", "GIGA"):
        with pytest.raises(ValueError, match="giga_geo"):
            trainer.GeoTrainer(None, [], net_name=name)
    with pytest.raises(ValueError):
        trainer.Trainer(None, [], net_name="vgn")
    assert issubclass(trainer.GeoTrainer, trainer.Trainer)
    assert trainer.GeoTrainer.score_key == "occ_accuracy" and trainer.Trainer.score_key == "accuracy"
    assert trainer.GeoTrainer.finalize is trainer.finalize_geo_metrics and trainer.Trainer.finalize is trainer.finalize_metrics
    import giga_amd
    from giga_amd import training
    assert giga_amd.GeoTrainer is trainer.GeoTrainer and giga_amd.geo_loss is training.geo_loss
    assert giga_amd.Trainer is trainer.Trainer


def test_geo_loss_refuses_host_tensors_and_wrong_shapes():
    from giga_amd.training import geo_loss
    with pytest.raises(_capi.GigaHipError):                  # no CPU fallback
        geo_loss(torch.zeros(2, 3), torch.zeros(2, 3))


def test_geo_model_has_the_training_switches():
    from giga_amd import convonet
    net = networks.get_network("giga_geo")
    assert isinstance(net, convonet.ConvolutionalOccupancyNetworkGeometry) and net._head_present() == 8
    for name in ("flatten_parameters", "set_train_precision", "enable_data_parallel", "packed_blob", "packed_bwd_blob"):
        assert getattr(type(net), name) is getattr(convonet.ConvolutionalOccupancyNetwork, name), name     # one copy, shared
    shapes = weights.giga_param_shapes(heads=("decoder_tsdf",))
    sd = weights.make_state_dict(3, heads=("decoder_tsdf",))
    net.load_state_dict(sd)
    (flat,) = net.flatten_parameters()
    assert flat.requires_grad and flat.numel() == sum(int(np.prod(s)) for s in shapes.values()) == _capi.lib().giga_param_count(8)
    assert net.flatten_parameters()[0] is flat and not any(q.requires_grad for q in net.parameters())
    assert list(net.state_dict()) == list(shapes)
    assert torch.equal(flat.detach(), torch.cat([v.reshape(-1) for v in sd.values()]))
    assert all(torch.equal(v, sd[k]) for k, v in net.state_dict().items())
    with torch.no_grad():
        flat[0] = 5.0                                        # the named parameters are views of the flat one
    assert next(iter(net.state_dict().values())).reshape(-1)[0] == 5.0
    assert net.set_train_precision("bf16") is net and net._train_bf16 and net._train_bf16_dec
    assert net.set_train_precision("fp32") is net and not net._train_bf16
    with pytest.raises(ValueError):
        net.set_train_precision("fp8")
    assert net.enable_data_parallel(None, True) is net and net._dp == (True, None)


# -------------------------------------------------------------------------------------------------------- checkpoints
def test_geo_checkpoint_files(tmp_path):
    net = networks.get_network("giga_geo")                   # a CPU module: only its state dict is written
    net.load_state_dict(weights.make_state_dict(3, heads=("decoder_tsdf",)))
    sd = net.state_dict()
    shapes = weights.giga_param_shapes(heads=("decoder_tsdf",))
    logdir = tmp_path / "run"
    ck = trainer.Checkpoints(logdir, "giga_geo")
    names = lambda: sorted(p.name for p in logdir.iterdir())  # noqa: E731
    first = ck.save_epoch(sd, 7)
    assert names() == ["vgn_giga_geo_7.pt"] and first == str(logdir / "vgn_giga_geo_7.pt")
    got = torch.load(first)
    assert list(got) == list(shapes) == list(sd)
    assert all(tuple(got[k].shape) == tuple(shapes[k]) and torch.equal(got[k], sd[k]) for k in shapes)
    assert Path(first).stem.split("_")[1:-1] == ["giga", "geo"]
    loaded = networks.load_network(first, "cpu")             # the model name from the file stem, as the reference's loader
    assert type(loaded) is type(net) and all(torch.equal(a, b) for a, b in zip(loaded.state_dict().values(), sd.values()))
    ck.save_epoch(sd, 14)
    assert names() == ["vgn_giga_geo_14.pt"] and ck.epoch_files() == [(14, str(logdir / "vgn_giga_geo_14.pt"))]
    assert ck.save_best(sd, 0.91237) == str(logdir / "best_vgn_giga_geo_val_acc=0.9124.pt")
    assert ck.save_best(sd, 0.9) is None and ck.save_best(sd, 0.95) is not None
    assert names() == ["best_vgn_giga_geo_val_acc=0.9500.pt", "vgn_giga_geo_14.pt"]
    assert list(torch.load(logdir / "best_vgn_giga_geo_val_acc=0.9500.pt")) == list(shapes)
    with pytest.raises(ValueError, match="resume"):
        trainer.Checkpoints(logdir, "giga_geo")


# -------------------------------------------------------------------------------------------------------- command line
def test_geo_parser_accepts_the_reference_command_line():
    parser = train_geo.build_parser()
    a = parser.parse_args(["--dataset", "data/set", "--dataset_raw", "data/set_raw"])
    assert (a.net, a.epochs, a.batch_size, a.lr, a.val_split) == ("giga_geo", 10, 32, 2e-4, 0.1)
    assert (a.augment, a.silence, a.load_path, a.description, a.savedir) == (False, False, "", "", "")
    assert a.dataset == Path("data/set") and a.dataset_raw == Path("data/set_raw") and Path(a.logdir) == Path("data/runs")
    assert (a.precision, a.seed, a.resume) == ("fp32", 0, False)
    b = parser.parse_args("--net giga_geo --dataset d --dataset_raw r --logdir runs --description try --savedir out --epochs 3 "
                          "--batch-size 16 --lr 1e-3 --val-split 0.2 --augment --silence --load-path w.pt --precision bf16 --seed 9 "
                          "--resume".split())
    assert (b.net, b.epochs, b.batch_size, b.lr, b.val_split, b.augment, b.silence) == ("giga_geo", 3, 16, 1e-3, 0.2, True, True)
    assert (b.load_path, b.precision, b.seed, b.resume, b.savedir) == ("w.pt", "bf16", 9, True, "out")
    for net in ("giga", "giga_aff", "giga_detach", "vgn"):   # the other nets are giga_amd.train's
        with pytest.raises(SystemExit):
            parser.parse_args(["--dataset", "d", "--dataset_raw", "r", "--net", net])
        with pytest.raises(SystemExit):
            train_geo.parse_args(["--dataset", "d", "--dataset_raw", "r", "--net", net])
    with pytest.raises(SystemExit):
        parser.parse_args(["--dataset", "d"])                # --dataset_raw is required
    with pytest.raises(SystemExit):
        train_geo.parse_args(["--dataset", "d", "--dataset_raw", "r", "--resume"])
    assert train_geo.parse_args(["--dataset", "d", "--dataset_raw", "r", "--resume", "--savedir", "out"]).resume is True
    assert train.run_directory(b) == Path("out")
    assert train.run_directory(a, datetime(2024, 3, 5, 14, 7)) == \
        Path("data/runs") / "24-03-05-14-07_dataset=set,augment=False,net=giga_geo,batch_size=32,lr=2e-04"
    # giga_amd.train's own parser is what it was: giga by default, any net name passes the parser
    t = train.build_parser().parse_args(["--dataset", "d", "--dataset_raw", "r"])
    assert t.net == "giga" and train.parse_args(["--dataset", "d", "--dataset_raw", "r", "--net", "giga_aff"]).net == "giga_aff"
    assert "train_giga_geo.py:124" in train_geo.__doc__ and "--augment" in train_geo.__doc__
