"""What does a giga_geo training step cost?  (run on the GPU box)

    PYTHONPATH=. python tools/gpu_geo_step_time.py [out.txt]

At the c5 shape (32 scenes, 2048 occupancy points), on one resident batch, in fp32 and bf16, times in ONE process, alternating,
each round of STEPS steps between two HIP events:
  geo     the step of `GeoTrainer`: net(x, None, p_tsdf=pos_occ), geo_loss with the epoch accumulator, backward, FlatAdam;
  torch   the form there was before the module could train: GigaFunction.apply on a _TrainState(8) over a hand-made flat parameter,
          F.binary_cross_entropy(torch.sigmoid(z), t, reduction="none").mean(-1).mean(), ignite's three metric reductions in torch
          (round, ==, products and sums into device counters), backward, FlatAdam;
  giga    the joint model's step (net, giga_loss with the accumulator, backward, FlatAdam), for scale."""
import statistics
import sys

import torch
import torch.nn.functional as F

from giga_amd import networks, synth, trainer, weights
from giga_amd.optim import FlatAdam
from giga_amd.training import GigaFunction, _TrainState, geo_loss, giga_loss

B, M, STEPS, ROUNDS = 32, 2048, 100, 5


def main():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda:0")
    x = torch.from_numpy(synth.tsdf_batch(0, B)).to(dev)
    pos = torch.from_numpy(synth.query_points(0, B, 1, stream=2, half_width=0.45)).to(dev)
    pos_occ = torch.from_numpy(synth.query_points(0, B, M, stream=3, half_width=0.45)).to(dev)
    y = tuple(torch.from_numpy(a).to(dev) for a in synth.train_labels(0, B, M))
    say(f"{torch.cuda.get_device_name(0)}; batch {B}, {M} occupancy points, {ROUNDS} alternating rounds of {STEPS} steps after a "
        f"warm-up round of each")

    geo = networks.get_network("giga_geo")
    geo.load_state_dict(weights.make_state_dict(7, heads=("decoder_tsdf",)))
    geo = geo.to(dev).train()
    geo_opt = FlatAdam(geo.flatten_parameters(), lr=2e-4)
    geo_acc = trainer.TrainMetrics(dev)

    def geo_step():
        geo_opt.zero_grad(set_to_none=True)
        loss, _ = geo_loss(geo(x, None, p_tsdf=pos_occ), y[3], metrics=geo_acc)
        loss.backward()
        geo_opt.step()

    flat = torch.cat([v.reshape(-1) for v in weights.make_state_dict(7, heads=("decoder_tsdf",)).values()]).to(dev).requires_grad_(True)
    state = _TrainState(8, dev)
    old_opt = FlatAdam([flat], lr=2e-4)
    counters = torch.zeros(5, device=dev)                    # correct, examples, tp, predicted positives, actual positives
    loss_sum = torch.zeros((), device=dev)
    no_grasp = torch.empty((B, 0, 3), device=dev)

    def torch_step():
        old_opt.zero_grad(set_to_none=True)
        (z,) = GigaFunction.apply(state, x, no_grasp, pos_occ, flat)
        p = torch.sigmoid(z)
        loss = F.binary_cross_entropy(p, y[3], reduction="none").mean(-1).mean()
        with torch.no_grad():
            pred = torch.round(p)
            counters[0] += (pred == y[3]).sum()
            counters[1] += pred.numel()
            counters[2] += (pred * y[3]).sum()
            counters[3] += pred.sum()
            counters[4] += y[3].sum()
            loss_sum.add_(loss.detach())
        loss.backward()
        old_opt.step()

    giga = networks.get_network("giga")
    giga.load_state_dict(weights.make_state_dict(7))
    giga = giga.to(dev).train()
    giga_opt = FlatAdam(giga.flatten_parameters(), lr=2e-4)
    giga_acc = trainer.TrainMetrics(dev)

    def giga_step():
        giga_opt.zero_grad(set_to_none=True)
        loss, _ = giga_loss(giga(x, pos, p_tsdf=pos_occ), y, metrics=giga_acc)
        loss.backward()
        giga_opt.step()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(STEPS):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / STEPS

    loops = {"geo": geo_step, "torch": torch_step, "giga": giga_step}
    for prec in ("fp32", "bf16"):
        geo.set_train_precision(prec)
        giga.set_train_precision(prec)
        state.bf16 = state.bf16_dec = prec == "bf16"
        state._wkey = None
        for fn in loops.values():
            timed(fn)
        ms = {k: [] for k in loops}
        for _ in range(ROUNDS):
            for k, fn in loops.items():
                ms[k].append(timed(fn))
        for k, v in ms.items():
            say(f"{prec} {k:6s} ms/step: median {statistics.median(v):.4f}  min {min(v):.4f}  max {max(v):.4f}  "
                f"[{' '.join(f'{t:.4f}' for t in v)}]")
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
