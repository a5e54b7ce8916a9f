"""What feeds the training step fastest?  (run on the GPU box)

    PYTHONPATH=. python tools/gpu_resident_feed_bench.py [n_scenes] [grasps_per_scene] [out.json]

Writes a synthetic training set in the reference's on-disk layout to a temporary directory (synth.write_training_set) and times,
in one run, at batch 32 and M = 2048, in bf16 and fp32:
  (a) the training step on FIXED resident inputs (bench.py's c5 step),
  (b) the step fed by eight reader processes through the shared-memory ring (GraspOccRing -> TSDFFeed), without and with the
      host-side augmentation,
  (c) the step fed by ResidentBatches (giga_amd.resident), without and with the device-side augmentation,
  (d) draw + assemble alone, by HIP events.
Fed figures are the mean over the epochs after the first (the first starts the readers and fills their caches)."""
import json
import sys
import tempfile
import time

import torch

from giga_amd import dataset, networks, resident, synth, weights
from giga_amd.feed import TSDFFeed
from giga_amd.training import giga_loss

B, M, EPOCHS = 32, 2048, 3


def main():
    n_scenes = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    gps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    out = {"batch": B, "occupancy_points": M}
    with tempfile.TemporaryDirectory() as tmp:
        root, raw = tmp + "/data", tmp + "/raw"
        n = synth.write_training_set(root, raw, n_scenes=n_scenes, grasps_per_scene=gps, occ_files=(2, 4), n_occ_points=20000, seed=9)
        sets = {aug: dataset.GraspOccDataset(root, raw, num_point_occ=M, augment=aug) for aug in (False, True)}
        # the reader processes are forked before this process touches the device
        rings = {aug: dataset.GraspOccRing(ds, B, workers=8, seed=2, drop_last=True) for aug, ds in sets.items()}
        dev = torch.device("cuda:0")
        t0 = time.perf_counter()
        rset = resident.ResidentTrainingSet(sets[False], device=dev)
        torch.cuda.synchronize()
        out["dataset"] = {"grasps": n, "scenes": n_scenes, "steps_per_epoch": n // B, "resident_bytes": rset.nbytes,
                          "resident_build_s": time.perf_counter() - t0}
        net = networks.get_network("giga"); net.load_state_dict(weights.make_state_dict(7)); net = net.to(dev)
        net.set_precision("fp32").train()
        opt = torch.optim.Adam(net.flatten_parameters(), lr=2e-4, fused=True)

        def step(x, pos, pos_occ, y):
            opt.zero_grad(set_to_none=True)
            loss, _ = giga_loss(net(x, pos, p_tsdf=pos_occ), y)
            loss.backward()
            opt.step()

        def epochs(make):
            """ms per step of every epoch of an iterable of (x, pos, pos_occ, y)"""
            ms = []
            for _ in range(EPOCHS):
                k = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for batch in make():
                    step(*batch)
                    k += 1
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) / max(k, 1) * 1e3)
            return {"first_epoch": ms[0], "steady": sum(ms[1:]) / len(ms[1:])}

        fixed = tuple(t.clone() if torch.is_tensor(t) else tuple(v.clone() for v in t)
                      for t in next(iter(resident.ResidentBatches(rset, B, seed=1, augment=False))))
        for prec in ("bf16", "fp32"):
            net.set_train_precision(prec)
            res = {}
            for _ in range(5):
                step(*fixed)
            torch.cuda.synchronize()
            K = 100
            t0 = time.perf_counter()
            for _ in range(K):
                step(*fixed)
            torch.cuda.synchronize()
            res["a_fixed_inputs_ms"] = (time.perf_counter() - t0) / K * 1e3
            for aug in (False, True):
                tag = "_augment" if aug else ""
                res["b_ring_8_procs" + tag + "_ms"] = epochs(
                    lambda: (dataset.network_inputs(b) for b in TSDFFeed(rings[aug], dev)))
                batches = resident.ResidentBatches(rset, B, seed=2, drop_last=True, augment=aug)
                res["c_resident" + tag + "_ms"] = epochs(lambda: batches)
            out[prec] = res
        net.set_train_precision("fp32")
        for ring in rings.values():
            ring.close()
        # (d) draw + assemble alone: HIP events around K batches.  The host enqueues slower than the device works through two
        # small kernels, so the stream is first held busy (a spin kernel) while the K batches queue up behind it: the events
        # then bracket device time only (`queued` says whether the host was done before the spin ended)
        ordinals, rows = (torch.from_numpy(a.astype("int32")).to(dev) for a in resident.epoch_order(range(len(rset)), 3, 1))
        spin = 400_000_000
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record(); torch.cuda._sleep(spin); ev[1].record()
        torch.cuda.synchronize()
        spin_ms = ev[0].elapsed_time(ev[1])
        alone = {"spin_ms": spin_ms}
        for aug in (False, True):
            for what in ("draw", "assemble", "draw_and_assemble"):
                draws = rset.draw(ordinals[:B], 1, 3, rows[:B], M)

                def once(k):
                    lo = (k * B) % (len(rset) - B + 1)
                    d = rset.draw(ordinals[lo:lo + B], 1, 3, rows[lo:lo + B], M) if what != "assemble" else draws
                    if what != "draw":
                        rset.assemble(rows[lo:lo + B] if what != "assemble" else rows[:B], d, M, aug)

                for k in range(10):
                    once(k)
                K = 200
                torch.cuda.synchronize()
                torch.cuda._sleep(spin)
                ev[0].record()
                t0 = time.perf_counter()
                for k in range(K):
                    once(k)
                host_ms = (time.perf_counter() - t0) * 1e3
                ev[1].record()
                torch.cuda.synchronize()
                alone[what + ("_augment" if aug else "")] = {"device_us": ev[0].elapsed_time(ev[1]) / K * 1e3, "host_enqueue_us": host_ms / K * 1e3,
                                                             "queued": host_ms < spin_ms}
        out["d_alone"] = alone
    line = json.dumps(out)
    print(line)
    if len(sys.argv) > 3:
        with open(sys.argv[3], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
