"""Does the Trainer's epoch cost anything over a bare loop?  (run on the GPU box)

    PYTHONPATH=. python tools/gpu_train_epoch_time.py [out.txt]

Writes a synthetic training set (synth.write_training_set: 64 scenes x 100 grasps, 20 000 occupancy points per file), makes it
resident, and at the c5 shape (32 scenes, 2048 occupancy points, 200 steps per epoch), in bf16 and fp32, times in ONE process
  (a) milliseconds per step of `Trainer.train_epoch` (metrics on the device, one copy at the end) against a bare loop over the same
      batches on net + giga_loss without metrics + backward + FlatAdam, and against that bare loop with the accumulator alone,
      alternating, each epoch between two HIP events; beside it the host's time to enqueue the epoch (for the Trainer that
      includes the wait of the metrics copy);
  (b) the mean launch of the loss with and without the epoch accumulator, alone between two HIP events on its own stream
      (giga_launch_probe), alternating, median of 50."""
import ctypes
import statistics
import sys
import tempfile
import time

import torch

from giga_amd import _capi, dataset, networks, resident, synth, trainer, weights
from giga_amd.optim import FlatAdam
from giga_amd.training import giga_loss

B, M, ROUNDS = 32, 2048, 5


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    L = _capi.lib()
    with tempfile.TemporaryDirectory() as tmp:
        root, raw = tmp + "/data", tmp + "/raw"
        n = synth.write_training_set(root, raw, n_scenes=64, grasps_per_scene=100, occ_files=(1, 2), n_occ_points=20000, seed=9)
        rset = resident.ResidentTrainingSet(dataset.GraspOccDataset(root, raw, num_point_occ=M, augment=True), device=dev)
    batches = resident.ResidentBatches(rset, B, shuffle=True, seed=2, drop_last=True)
    steps = len(batches)
    say(f"{torch.cuda.get_device_name(0)}; {n} grasps resident ({rset.nbytes / 1e6:.1f} MB), batch {B}, {M} occupancy points, "
        f"{steps} steps per epoch, {ROUNDS} alternating rounds after one warm-up epoch of each")
    net = networks.get_network("giga"); net.load_state_dict(weights.make_state_dict(7)); net = net.to(dev)
    tr = trainer.Trainer(net, batches, quiet=True)
    opt = FlatAdam(net.flatten_parameters(), lr=2e-4)

    def bare_epoch():
        net.train()
        for x, pos, pos_occ, y in batches:
            opt.zero_grad(set_to_none=True)
            loss, _ = giga_loss(net(x, pos, p_tsdf=pos_occ), y)
            loss.backward()
            opt.step()

    probe = trainer.TrainMetrics(dev)

    def metrics_epoch():                                     # the bare loop with the accumulator alone: isolates the loss launch
        net.train()
        probe.reset()
        for x, pos, pos_occ, y in batches:
            opt.zero_grad(set_to_none=True)
            loss, _ = giga_loss(net(x, pos, p_tsdf=pos_occ), y, metrics=probe)
            loss.backward()
            opt.step()

    def timed(fn):
        """(ms per step between two HIP events, ms per step the host took to enqueue the epoch)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        host = time.perf_counter() - t0
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps, host * 1e3 / steps

    for prec in ("bf16", "fp32"):
        net.set_train_precision(prec)
        bare_epoch()
        tr.train_epoch()
        metrics_epoch()
        loops = {"bare": bare_epoch, "bare+acc": metrics_epoch, "trainer": tr.train_epoch}
        ms, host = {k: [] for k in loops}, {k: [] for k in loops}
        for _ in range(ROUNDS):
            for k, fn in loops.items():
                t, h = timed(fn)
                ms[k].append(t)
                host[k].append(h)
        for k, v in ms.items():
            say(f"{prec} {k:8s} ms/step: mean {statistics.mean(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  "
                f"[{' '.join(f'{t:.4f}' for t in v)}]  host enqueue {statistics.mean(host[k]):.4f}")
        spread = max(ms["bare"]) - min(ms["bare"])
        say(f"{prec} trainer - bare: {statistics.mean(ms['trainer']) - statistics.mean(ms['bare']):+.4f} ms/step "
            f"(spread of the bare loop itself: {spread:.4f})")

    # (b) the mean launch alone: the second launch of the loss call, bracketed on its own stream
    x, pos, pos_occ, y = next(iter(batches))
    with torch.no_grad():
        out = net.eval()(x, pos, p_tsdf=pos_occ)
    args = [t.contiguous().float() for t in out + y]
    losses, scene = torch.empty(5, device=dev), torch.empty((B, 5), device=dev)
    acc = trainer.TrainMetrics(dev)
    ev = (L.giga_event_create(), L.giga_event_create())
    ptrs = [_capi.ptr(t) for t in args]

    def mean_launch_us(with_acc):
        L.giga_launch_probe(L.giga_launch_count() + 2, ev[0], ev[1])
        if with_acc:
            _capi.check(L.giga_train_loss_metrics(*ptrs, B, M, _capi.ptr(losses), _capi.ptr(scene), _capi.ptr(acc.acc), _capi.stream_ptr(dev)), "loss")
        else:
            _capi.check(L.giga_train_loss(*ptrs, B, M, _capi.ptr(losses), _capi.ptr(scene), _capi.stream_ptr(dev)), "loss")
        t = ctypes.c_float()
        _capi.check(L.giga_event_elapsed_ms(ev[0], ev[1], ctypes.byref(t)), "event")
        name = (L.giga_launch_probe_name() or b"").decode()
        L.giga_launch_probe(0, None, None)
        return t.value * 1e3, name

    us = {False: [], True: []}
    names = {}
    for i in range(55):
        for with_acc in (False, True):
            t, names[with_acc] = mean_launch_us(with_acc)
            if i >= 5:
                us[with_acc].append(t)
    for with_acc in (False, True):
        v = us[with_acc]
        say(f"mean launch {'with' if with_acc else 'without'} the accumulator ({names[with_acc]}): median {statistics.median(v):.2f} us  "
            f"min {min(v):.2f}  max {max(v):.2f}  (50 launches between HIP events)")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
