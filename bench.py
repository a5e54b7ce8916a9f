#!/usr/bin/env python
"""Benchmark of the GIGA dense inference path on MI355X (driver contract in the task brief).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full [--no-extra] [--no-cpu-baseline]]

With N > 1 and no launcher environment the script starts its own N ranks (`python -m torch.distributed.run`, one per GPU,
rendezvous on 127.0.0.1) and rank 0 prints the JSON line; under an external `torch.distributed.run` it uses the ranks it
is given.  WORLD_SIZE must equal --gpus.

A "step" is one forward pass of BASELINE.json configs[1] on every rank:
    32 synthetic 40^3 TSDF scenes per GPU, the literal `train_giga` call shape
    (1 grasp query point for the three grasp heads + 2048 occupancy queries per scene),
    encoder + decoders in exact fp32 (fp32 MFMA), inputs resident in HBM, outputs left in HBM.
Scenes are independent, so ranks are pure replicas on different scenes (scene i -> rank i mod N, weak scaling) and the
timed region has no collective; its two barriers run over gloo.  After it an RCCL group (backend "nccl" over xGMI) does the
MAX-reduce of the elapsed times and one all_gather of per-rank counters; with --full also the all_gather of the real head
outputs of all N x 32 scenes (BASELINE config c3) and, at N > 1, the data-parallel training step of config c5.

A plain run does only what the headline needs: set-up, warm-up, the timed steps, --dump-outputs and ONE JSON line (< 6 KB),
printed by rank 0: the contract keys, and
  roofline      - the headline kernel of the timed workload (scalars only), timed live with HIP events on the launch stream
                  inside the timed steps
  launches_per_step, rccl_ranks / per_rank_seconds at N > 1
  summary       - ms per step and roofline fraction of every BASELINE config the run measured (last key)
--full adds everything else the benchmark measures or checks: before the timed region the untimed pre-pass (`roofline.stages`:
time, FLOPs and fraction of peak of EVERY kernel; a plain run makes it only when the U-Net runs one launch per layer, to pick
the kernel the timed steps bracket), after it `checked_vs_oracle` (scene 0 of the headline step against the CPU oracle), the
other configs and precisions (the c4 legs: 64 000 grasp queries per scene, f16 / f16x3 / mixed; c2 (ii); c2 in fp16x3; the
c5-shaped training steps with their per-kernel tables; at N > 1 the c3 gather and the data-parallel c5 step, whose digests join
the line) and, at N = 1, `cpu_baseline` (the CPU oracle, a port of the reference's PyTorch path, on the host cores).
--no-extra / --no-cpu-baseline leave the other configs / the CPU baseline out of a --full run.  Everything beyond the line goes
to the side file bench_extra.json (GIGA_BENCH_EXTRA sets its path, see emit()), never to stdout: round 5's 31-KB line could not
be parsed.

--dump-outputs DIR writes what the LAST timed step returned (rank 0's shard: qual, rot, width, tsdf) as DIR/<name>.npy in
float32, so that two builds can be compared output for output; the inputs and weights are seeded, identical from run to run.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_F32_MATRIX_TFLOPS = 157.3        # MI355X_MICROARCH.md: fp32-input MFMA == fp32 vector peak
PEAK_F16_MFMA_TFLOPS = 2500.0         # dense f16/bf16 MFMA
PEAK_HBM_GBS = 8000.0                 # HBM3E
# Sustained peaks measured on the round-1 box by tools/mfma_peak.hip (profiles/r01j_hw_peaks.txt): back-to-back
# register-resident MFMAs on all 1024 SIMDs.  Reported beside the spec fraction; `frac` stays spec-based.
MEASURED_F32_MATRIX_TFLOPS = 156.3    # v_mfma_f32_32x32x2_f32 (99.4 % of spec)
MEASURED_F16_MFMA_TFLOPS = 2350.6     # v_mfma_f32_32x32x16_f16 (94 % of spec: the matrix-core clock sags to 2.24 GHz)
FLOP_ENCODER = 1_132_953_600          # SURVEY.md 8d / BASELINE.md section 4
FLOP_HEAD = {"qual": 51_456, "rot": 51_648, "width": 51_456, "tsdf": 51_456}
FLOP_GRASP3 = 154_560
# Lattice decoder (decoder_lat_kernel): f16 MFMA instructions (32x32x16: 32 768 FLOP) ISSUED per 32-point tile and head -- 43 in the
# plain mode, 107 in f16x3, plus the slab's line jobs (22 jobs of 3 / 7 (9 / 19) MFMAs per 50 tiles) -- against the 1 648 640
# ALGORITHMIC FLOP of that tile and head: two thirds of fc_c are evaluated once per plane pixel, not per point.
ISSUED_PER_ALGORITHMIC = {"fp16": (43 + 1.8) * 32768 / (32 * 51_520.0), "fp16x3": (107 + 5.3) * 32768 / (32 * 51_520.0)}

# U-Net layer table (kind, cin, cout, H, W): algorithmic FLOPs per image = 2*H*W*taps*cin*cout
_CONV = [(9, 32, 32, 40), (9, 32, 32, 40), (9, 32, 64, 20), (9, 64, 64, 20), (9, 64, 128, 10), (9, 128, 128, 10),
         (4, 128, 64, 10), (9, 128, 64, 20), (9, 64, 64, 20), (4, 64, 32, 20), (9, 64, 32, 40), (9, 32, 32, 40),
         (1, 32, 32, 40)]
STAGE_NAMES = ["convin_project", "plane_finalize"] + [
    "unet.down0.conv1", "unet.down0.conv2+pool", "unet.down1.conv1", "unet.down1.conv2+pool", "unet.down2.conv1",
    "unet.down2.conv2", "unet.up0.upconv", "unet.up0.conv1", "unet.up0.conv2", "unet.up1.upconv",
    "unet.up1.conv1", "unet.up1.conv2", "unet.conv_final",
    "unet (one persistent launch: 12 layers)"]                 # probe stage 15 = the whole U-Net, however it is launched
UNET_STAGE = 15
HEADLINE_STAGE = 9                      # unet.up0.conv1: the layer with the most FLOPs (5.66 GFLOP at 32 scenes) and, since the
                                        # round-2 conv_in rewrite, the longest launch of the step; see pick_headline()
NAMED_STAGE = 0                         # convin_project: the kernel VERDICT r01 names; reported beside it (roofline.r01_kernel)


# kernel-name fragments (rocprofv3 names) of the stages whose HBM traffic bench.py quotes from the committed PMC tables
TRAFFIC_KERNEL = {"convin_project": "convin_project_kernel<float, 5, false",
                  "unet (one persistent launch: 12 layers)": "unet_mega_kernel<float, 0",
                  "unet.up0.conv1": "conv16_kernel<float, 0, 64, 64, 64, 20, 20, 1, false, true, 0>",
                  "unet.up1.conv1": "conv16_kernel<float, 0, 32, 32, 32, 40, 40, 2, false, true, 0>"}


def traffic_lookup(workload, fragment):
    """HBM bytes per launch of the kernel whose name contains `fragment`, from profiles/r0N_traffic_<workload>.json (two
    rocprofv3 PMC passes, tools/gpu_traffic.sh): PMC counters cannot be collected from inside this process.  Returns
    (bytes or None, provenance or None)."""
    if not fragment:
        return None, None
    for rnd in ("r06", "r05", "r04", "r03", "r02"):               # the newest committed table that knows the kernel
        try:
            tab = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_traffic_{workload}.json")))
        except (OSError, ValueError):
            continue
        for name, ent in tab.get("kernels", {}).items():
            if fragment in name:
                return ent["bytes"], {"table": f"profiles/{rnd}_traffic_{workload}.json", "commit": tab.get("commit"), "kernel": name,
                                      "fetch_kib": ent["fetch_kib"], "write_kib": ent["write_kib"]}
    return None, None


def traffic_c5(precision):
    """HBM bytes of ONE c5 training step (every kernel of it) from profiles/r0N_traffic_c5.json, and the five kernels that move the
    most.  Returns (bytes or None, provenance or None)."""
    for rnd in ("r06", "r05"):
        try:
            tab = json.load(open(os.path.join(ROOT, "profiles", f"{rnd}_traffic_c5.json")))["bf16" if precision.startswith("bf16") else "fp32"]
        except (OSError, ValueError, KeyError):
            continue
        top = sorted(tab["kernels"].items(), key=lambda kv: -kv[1]["bytes_per_step"])[:5]
        return tab["bytes_per_step"], {"table": f"profiles/{rnd}_traffic_c5.json", "commit": tab.get("commit"),
                                       "five_heaviest_kernels": [{"kernel": k.split("(")[0][-80:], "MB_per_step": round(v["bytes_per_step"] / 1e6, 2),
                                                                  "launches_per_step": v["launches_per_step"]} for k, v in top]}
    return None, None


def stage_flops(stage, B):
    """Algorithmic FLOPs of one launch of encoder stage `stage` for B scenes."""
    if stage == 0:
        return 110_592_000 * B
    if stage == 1:
        return 0
    if stage == UNET_STAGE:                                     # the twelve layers of the folded call (conv_final is not run)
        return sum(stage_flops(st, B) for st in range(2, 14))
    taps, cin, cout, hw = _CONV[stage - 2]
    return 2 * hw * hw * taps * cin * cout * 3 * B


def unet_issued_flops(B):
    """fp32 MFMA FLOPs the U-Net launch ISSUES for B scenes in its default form (csrc/giga_wino.h): the ten 3x3 layers as Winograd
    F(2x2, 3x3) -- 16 positions x cin / 4 K-steps of v_mfma_f32_16x16x4_f32 (2048 FLOP) per (block of <= 16 tiles, 16 output channels),
    blocks of 4 x 4 tiles on the 40^2 images (all full), of 5 x 3 on the 20^2 / 10^2 ones (8 / 2 blocks per image for 100 / 25 tiles) --
    and the two ConvTranspose layers as four plain GEMMs per 16 pixels.  `roofline.achieved` counts the ALGORITHMIC (direct-convolution)
    FLOPs of SURVEY 8d; this is what keeps the matrix pipe busy."""
    nimg, fl = 3 * B, 0
    for taps, cin, cout, hw in _CONV[:12]:
        if taps == 9:
            tw = hw // 2
            blocks = (tw // 4) ** 2 if tw % 4 == 0 else -(-tw // 5) * -(-tw // 3)
            fl += nimg * blocks * (cout // 16) * 16 * (cin // 4) * 2048
        elif taps == 4:
            fl += -(-nimg * hw * hw // 16) * (cout // 16) * 4 * (cin // 4) * 2048
    return fl


def pick_headline(stage_ms):
    """Deterministic choice of the roofline kernel = the dominant (longest) launch of the step: unet.up0.conv1, the layer
    with the most FLOPs, unless another stage takes more than 1.15x its time (a plain argmax flips between runs when two
    stages sit within a microsecond of each other, as up0.conv1 and up1.conv1 do)."""
    top = int(np.argmax(stage_ms))
    return HEADLINE_STAGE if stage_ms[HEADLINE_STAGE] * 1.15 >= stage_ms[top] else top


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n):
    """`python bench.py --gpus N` without a launcher: start N ranks ourselves and relay rank 0's JSON line."""
    have = torch.cuda.device_count()
    if have < n:
        raise SystemExit(f"--gpus {n} but only {have} HIP device(s) are visible")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32, help="scenes per GPU per step")
    ap.add_argument("--full", action="store_true", help="also the stage pre-pass, the oracle check, the other configs and "
                                                         "precisions and the CPU baseline (see the module docstring)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: without the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: without the other configs and precisions")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write the last timed step's outputs to DIR/<name>.npy (float32)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    launched = "RANK" in os.environ and "MASTER_PORT" in os.environ
    if args.gpus > 1 and not launched:
        spawn_ranks(args.gpus)
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1")) if launched else 1
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: one rank per GPU, WORLD_SIZE must equal --gpus")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (MI355X); no CPU fallback for the timed path")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if launched:
        # one rank per GPU (also at world size 1, so that the whole N > 1 code path runs on a single-GPU box).
        # Rendezvous and the barriers that bracket the timed region run over gloo (host side, TCP on 127.0.0.1); the
        # RCCL communicator for the collectives proper is created AFTER the timed region: the hot path has no collective,
        # and a live RCCL communicator (its streams / hardware queues) was measured to slow the single-GPU step by 2-5 %
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")    # one node by contract; the hostname may not resolve
        dist.init_process_group("gloo", rank=rank, world_size=world)

    from giga_amd import _capi, networks, sharding, synth, weights
    from giga_amd.convonet import decode_heads

    B, M = args.batch, 2048
    sd = weights.make_state_dict(7)
    net = networks.get_network("giga")
    net.load_state_dict(sd)
    net = net.to(dev).eval().set_precision("fp32")
    mine = sharding.scene_shard(world * B, rank, world)  # scene i -> rank i mod world (giga_amd/sharding.py)
    x = torch.from_numpy(synth.tsdf_scenes(mine)).to(dev)
    pos = torch.from_numpy(synth.query_points_for(mine, 1, stream=2)).to(dev)
    pos_occ = torch.from_numpy(synth.query_points_for(mine, M, stream=3)).to(dev)
    blob = net.packed_blob(dev)
    L = _capi.lib()

    def barrier():
        # drain the device first, so that the barrier is entered with an idle device on every rank
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    def step(probe=None, dec_probe=None):
        """One forward of the workload through the module API (vgn-compatible call)."""
        with torch.no_grad():
            if dec_probe is None:
                return net(x, pos, p_tsdf=pos_occ, _probe=probe)
            nhwc, _ = net.encoder.encode_nhwc(x, blob=blob, precision="fp32", fold_final=True)
            g = decode_heads(nhwc, pos, blob, 7, "fp32", True, probe=dec_probe[0], folded=True)
            t = decode_heads(nhwc, pos_occ, blob, 8, "fp32", False, probe=dec_probe[1], folded=True)
        return g, t

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    n0 = L.giga_launch_count()
    step()
    launches_per_step = int(L.giga_launch_count() - n0)       # kernels the library enqueues for one step (no profiler needed)
    ms = ctypes.c_float()

    def elapsed(a, b):
        _capi.check(L.giga_event_elapsed_ms(a, b, ctypes.byref(ms)), "event")
        return ms.value

    # How the U-Net is launched in the product call: one persistent launch (the default from 8 scenes up in fp32) or one launch per
    # layer.  Probing a single layer (stages 2..14) forces per-layer launches for that call, so the per-layer table below is always
    # available; the dominant launch of the STEP AS TIMED is the persistent one when it is in use.
    torch.cuda.synchronize()
    n0 = L.giga_launch_count()
    with torch.no_grad():
        net.encoder.encode_nhwc(x, blob=blob, precision="fp32", fold_final=True)
    persistent_unet = int(L.giga_launch_count() - n0) <= 4         # conv_in, finalize, U-Net

    # -------- untimed pre-pass (--full, or to pick the bracketed kernel of the per-layer form): every stage probed, median of seven
    stage_ms = dec_grasp_ms = dec_occ_ms = unet_ms = bracket_ms = None
    if args.full or not persistent_unet:
        ev_a, ev_b = L.giga_event_create(), L.giga_event_create()
        dec_ev = (L.giga_event_create(), L.giga_event_create())
        bracket_ms = empty_bracket_ms(L, _capi, dev)          # what an event pair costs with nothing between its records
        stage_ms = []
        for st in range(15):
            reps = []
            for _ in range(7):
                step(probe=(st, ev_a, ev_b))
                reps.append(elapsed(ev_a, ev_b))
            stage_ms.append(float(np.median(reps)))
        dec2 = (L.giga_event_create(), L.giga_event_create())
        dg, dt = [], []
        for _ in range(7):
            step(dec_probe=(dec_ev, dec2))
            dg.append(elapsed(*dec_ev)); dt.append(elapsed(*dec2))
        dec_grasp_ms, dec_occ_ms = float(np.median(dg)), float(np.median(dt))
        reps = []
        for _ in range(7):
            step(probe=(UNET_STAGE, ev_a, ev_b))
            reps.append(elapsed(ev_a, ev_b))
        unet_ms = float(np.median(reps))
    dom = UNET_STAGE if persistent_unet else pick_headline(stage_ms)

    # -------- timed region ----------------------------------------------------------------------------
    _settle()                              # (before the warm-up: an idle GPU drops its clocks ...
    for _ in range(40):                    # ... and these untimed steps, ~20 ms of GPU work, bring them back)
        step()
    for _ in range(args.warmup):
        step()
    K = args.steps
    evs = [(L.giga_event_create(), L.giga_event_create()) for _ in range(K)]
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(K + 1)]     # per-step durations (torch's current stream
    barrier()                                                                # is the stream the kernels are launched on)
    t0 = time.perf_counter()
    for i in range(K):
        marks[i].record()
        # even steps bracket the dominant kernel, odd steps the kernel VERDICT r01 names (conv_in + projection)
        last = step(probe=(dom if i % 2 == 0 else NAMED_STAGE, evs[i][0], evs[i][1]))
    marks[K].record()
    barrier()
    elapsed_s = time.perf_counter() - t0
    dom_ms, named_ms = [], []
    for i, (a, b) in enumerate(evs):
        (dom_ms if i % 2 == 0 else named_ms).append(elapsed(a, b))
        L.giga_event_destroy(a); L.giga_event_destroy(b)
    named_ms = named_ms or dom_ms
    step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(K)]
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, dict(zip(("qual", "rot", "width", "tsdf"), last)))
    del last
    if os.environ.get("GIGA_BENCH_DUMP_STEPS"):            # diagnosis: which of the K steps are the slow ones
        print("step_ms", " ".join(f"{v:.4f}" for v in step_ms), "| wall", f"{elapsed_s * 1e3:.4f}", "ms", file=sys.stderr)
    t_elapsed = torch.tensor([elapsed_s], dtype=torch.float64, device=dev)
    rccl = None
    multi = {}
    if dist is not None:
        rccl = dist.new_group(backend="nccl")                # one rank per GPU over RCCL / xGMI
        if dist.get_world_size(rccl) != args.gpus:
            raise SystemExit(f"RCCL group has {dist.get_world_size(rccl)} ranks, expected {args.gpus}")
        dist.all_reduce(t_elapsed, op=dist.ReduceOp.MAX, group=rccl)
        # the north-star's single data-path-free collective: gather per-rank counters
        counters = torch.tensor([float(B * K), elapsed_s, float(torch.cuda.current_device())], dtype=torch.float64, device=dev)
        gathered = [torch.zeros_like(counters) for _ in range(world)]
        dist.all_gather(gathered, counters, group=rccl)
        total_scenes = sum(float(c[0]) for c in gathered)
        if len({int(c[2]) for c in gathered}) != world and world > 1:
            raise SystemExit("two ranks share a GPU")
        multi["rccl_ranks"] = dist.get_world_size(rccl)
        multi["per_rank_seconds"] = [float(c[1]) for c in gathered]
    else:
        total_scenes = float(B * K)
    T = float(t_elapsed.item())
    scenes_per_s = total_scenes / T

    def finish():                          # every rank leaves together: no rank tears the communicator down early
        if dist is not None:
            import threading
            t = threading.Timer(60.0, lambda: os._exit(3))   # (a rank that died must not keep the others here for ever; rc != 0)
            t.daemon = True
            t.start()
            dist.barrier()
            dist.destroy_process_group()
            t.cancel()

    # The contract line is assembled BEFORE the multi-GPU extras run, and a watchdog prints it if they hang: a collective
    # that one rank never enters (an exception elsewhere, a wedged RCCL ring) must not cost the scaling run its numbers.
    out = core_result(args, world, B, M, K, T, scenes_per_s, stage_ms, dec_grasp_ms, dec_occ_ms, dom, dom_ms, step_ms, named_ms, bracket_ms,
                      launches_per_step, unet_ms, persistent_unet) if rank == 0 else None
    if rank == 0 and args.full:            # (untimed) scene 0 of the headline step's own output against the CPU oracle
        out["checked_vs_oracle"] = check_c2_scene(step(), sd, x, pos, pos_occ)
    extra = dict(multi)
    other_configs = args.full and not args.no_extra
    if dist is not None and other_configs:
        import threading

        def bail():
            if rank == 0:
                extra["multi_gpu_extras"] = "timed out after 240 s (a collective did not complete); core numbers are unaffected"
                out["extra"] = extra
                out["error"] = "watchdog: a multi-GPU extra (c3 gather / data-parallel step) hung; the process exits with rc 4"
                print(emit(out), flush=True)
            os._exit(4)                                      # a hang is a failure: never report rc 0

        dog = threading.Timer(240.0, bail)
        dog.daemon = True
        dog.start()
        try:
            extra["c3_gather"] = bench_c3_gather(net, x, pos, pos_occ, sharding, dist, rccl, rank, world, B, dev)
        except Exception as e:  # noqa: BLE001
            extra["c3_gather"] = {"error": f"{type(e).__name__}: {e}"}
        try:
            net.enable_data_parallel(group=rccl)
            for prec in ("bf16", "fp32"):                    # BASELINE c5 names bf16; the fp32 step beside it
                extra[f"c5_train_step_{prec}_data_parallel"] = bench_train(net, dev, synth, B, M, rank=rank, world=world,
                                                                              sync=barrier, precision=prec)
        except Exception as e:  # noqa: BLE001
            extra["c5_train_step_data_parallel_error"] = f"{type(e).__name__}: {e}"
        finally:
            net.enable_data_parallel(enabled=False)
            net.eval().set_precision("fp32")
        dog.cancel()

    if rank != 0:
        finish()
        return

    single = world == 1 and dist is None
    if single and other_configs:
        legs = (("c4", lambda: bench_c4_all(net, dev, L, _capi, synth, decode_heads)),
                ("c2_ii", lambda: bench_c2_ii(net, dev, synth, B)),
                ("c2_fp16x3", lambda: bench_c2_mode(net, x, pos, pos_occ, "fp16x3")),
                ("c5_train_step_fp32_param_list", lambda: bench_train(net, dev, synth, B, M, flat=False)),
                ("c5_train_step_fp32", lambda: bench_train(net, dev, synth, B, M)),
                ("c5_train_step_bf16", lambda: bench_train(net, dev, synth, B, M, precision="bf16")),
                ("c5_train_step_fp32_flat_adam", lambda: bench_train(net, dev, synth, B, M, giga_adam=True)),
                ("c5_train_step_bf16_flat_adam", lambda: bench_train(net, dev, synth, B, M, precision="bf16", giga_adam=True)))
        for key, fn in legs:
            try:
                r = fn()
                if key == "c4":
                    extra.update(r)
                else:
                    extra[key] = r
            except Exception as e:  # noqa: BLE001
                extra[key + "_error"] = f"{type(e).__name__}: {e}"
    if extra:
        out["extra"] = extra

    # -------- CPU baseline: the oracle (port of the reference path) on the host cores -------------------
    if single and args.full and not args.no_cpu_baseline:  # rank 0 at N = 1 only
        out["cpu_baseline"] = cpu_baseline(sd, synth, M)
    out["summary"] = summary_of(out)                      # LAST key: every named-config number inside the tail of the line
    print(emit(out), flush=True)
    finish()


DUMP_LIMIT = 64 << 20                      # bytes: --dump-outputs keeps a fixed sample of scenes beyond this


def dump_outputs(path, outs):
    """--dump-outputs: every output of the timed step as <path>/<name>.npy (float32, scenes along axis 0).  Should they exceed
    DUMP_LIMIT, the same fixed, seeded sample of scenes is kept of each, and its indices are written to scene_index.npy."""
    arrs = {k: v.detach().float().cpu().numpy() for k, v in outs.items()}
    n = len(next(iter(arrs.values())))
    per_scene = sum(a.nbytes for a in arrs.values()) / n
    budget = DUMP_LIMIT - 4096                                     # (the .npy headers)
    if per_scene * n > budget:
        keep = np.sort(np.random.default_rng(0).choice(n, size=max(1, int(budget // (per_scene + 8))), replace=False))
        arrs = {k: a[keep] for k, a in arrs.items()}
        arrs["scene_index"] = keep.astype(np.float64)
    os.makedirs(path, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(path, k + ".npy"), a)


LINE_LIMIT = 6144                          # bytes: the driver parses ONE line; round 5's 31-KB line came back as parsed = null
ROOFLINE_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "flops_per_launch")
CPU_BASELINE_KEYS = ("value", "unit", "cores", "kind", "sample")
CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config")


def contract_line(full):
    """The printed line: the driver contract's keys, a flat `roofline` (scalars only), `cpu_baseline`, `checked_vs_oracle`, the
    multi-GPU counters and `summary` -- nothing else.  Per-stage tables, the c4 / c5 legs and their notes live in the side file."""
    line = {k: full[k] for k in CONTRACT_KEYS if k in full}
    if full.get("roofline"):
        line["roofline"] = {k: full["roofline"].get(k) for k in ROOFLINE_KEYS}
    if full.get("cpu_baseline"):
        line["cpu_baseline"] = {k: full["cpu_baseline"].get(k) for k in CPU_BASELINE_KEYS}
    for k in ("checked_vs_oracle", "launches_per_step", "error"):
        if k in full:
            line[k] = full[k]
    ex = full.get("extra") or {}
    for k in ("rccl_ranks", "per_rank_seconds", "multi_gpu_extras"):
        if k in ex:
            line[k] = ex[k]
    for k in ("c3_gather", "c5_train_step_bf16_data_parallel", "c5_train_step_fp32_data_parallel"):      # N > 1: a digest of each
        v = ex.get(k)
        if isinstance(v, dict):
            line[k] = {q: v[q] for q in ("ms_per_step", "scenes_per_sec", "all_gather_ms", "scenes", "own_rows_match_on_every_rank",
                                         "launches_per_step", "error") if q in v}
    if "extra_file" in full:
        line["extra_file"] = full["extra_file"]
    if "summary" in full:
        line["summary"] = full["summary"]
    return line


def emit(full, path=None):
    """Write everything measured to the side file (gpurun_out/bench_extra.json, merged back from the GPU box) and return the
    contract line for stdout (< LINE_LIMIT bytes; the summary is shed key by key should it ever not fit)."""
    path = path or os.environ.get("GIGA_BENCH_EXTRA", os.path.join(ROOT, "gpurun_out", "bench_extra.json"))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            json.dump(full, f, indent=1)
        full["extra_file"] = os.path.relpath(path, ROOT)
    except OSError as e:                                  # a read-only tree must not cost the run its line
        print(f"bench.py: side file not written ({e})", file=sys.stderr)
    line = contract_line(full)
    text = json.dumps(line)
    while len(text) >= LINE_LIMIT and line.get("summary"):
        line["summary"].pop(next(reversed(line["summary"])))
        text = json.dumps(line)
    return text


def summary_of(out):
    """Compact digest of the line (its last key): ms per step / pass of every BASELINE config the run measured and the roofline
    fractions, so that a reader of the line's tail sees all of them."""
    ex = out.get("extra", {})
    g = lambda d, *ks: (lambda v: round(v, 4) if isinstance(v, float) else v)(_dig(d, ks))  # noqa: E731
    s = {"c2_fp32_ms": round(out["ms_per_step"], 4), "c2_scenes_per_s": round(out["value"], 1),
         "c2_unet_launch_frac_fp32_peak": g(out, "roofline", "frac"), "c2_unet_issued_mfma_frac": g(out, "roofline", "issued_mfma_frac_of_peak"),
         "c2_launches": out.get("launches_per_step"),
         "c2_fp16x3_ms": g(ex, "c2_fp16x3", "ms_per_step"), "c2_ii_fp32_ms": g(ex, "c2_ii", "fp32", "ms_per_step"),
         "c2_ii_fp16x3_ms": g(ex, "c2_ii", "fp16x3", "ms_per_step")}
    for k, v in ex.items():
        if k.startswith("c4") and isinstance(v, dict):
            s[k + "_ms"] = g(v, "ms_per_step") if "ms_per_step" in v else g(v, "ms_per_call")
            fr = _dig(v, ("roofline", "frac"))
            if fr is not None:
                s[k + "_decoder_frac"] = round(fr, 4)
        if k.startswith("c5_train_step") and isinstance(v, dict):
            s[k + "_ms"] = g(v, "ms_per_step")
            s[k + "_launches"] = v.get("launches_per_step")
            fr = _dig(v, ("roofline", "frac"))
            if fr is not None:
                s[k + "_frac"] = round(fr, 4)
    cb = out.get("cpu_baseline")
    if cb:
        s["cpu_scenes_per_s"] = round(cb["value"], 2)
        s["cpu_cores"] = cb["cores"]
    return s


def _dig(d, ks):
    for k in ks:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


def core_result(args, world, B, M, K, T, scenes_per_s, stage_ms, dec_grasp_ms, dec_occ_ms, dom, dom_ms, step_ms, named_ms, bracket_ms,
                launches_per_step=None, unet_ms=None, persistent_unet=False):
    """The contract keys + roofline of the timed region (rank 0); with the pre-pass's numbers (stage_ms not None) also its
    table of every stage (stage_report)."""
    # HBM bytes per launch: PMC counters cannot be collected from inside this process, so they come from the committed
    # rocprofv3 PMC table of the same workload (tools/gpu_traffic.sh -> profiles/*traffic_c2.json), stamped with the commit
    # and kernel it was measured on; null when the table has no entry for this kernel / batch size.
    traffic, traffic_src = traffic_lookup("c2", TRAFFIC_KERNEL.get(STAGE_NAMES[dom])) if B == 32 else (None, None)
    dom_avg_ms = float(np.mean(dom_ms))
    dom_flops = stage_flops(dom, B)
    named_avg_ms, named_flops = float(np.mean(named_ms)), stage_flops(NAMED_STAGE, B)
    named_traffic, named_src = traffic_lookup("c2", TRAFFIC_KERNEL.get(STAGE_NAMES[NAMED_STAGE])) if B == 32 else (None, None)
    named_ach = named_flops / (named_avg_ms * 1e-3) / 1e12
    achieved = dom_flops / (dom_avg_ms * 1e-3) / 1e12
    flop_scene = FLOP_ENCODER + FLOP_GRASP3 * 1 + FLOP_HEAD["tsdf"] * M
    points_per_scene = 1 * 3 + M          # head evaluations per scene
    out = {
        "metric": "scenes/sec",
        "value": scenes_per_s,
        "unit": "scenes/s",
        "n_gpus": world,
        "steps": K,
        "warmup": args.warmup,
        "ms_per_step": T / K * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {"workload": "c2: batch=32/GPU synthetic 40^3 TSDF, encoder + 3 grasp heads @1 query + "
                               "occupancy head @2048 queries/scene (literal train_giga call), fp32 MFMA",
                   "scenes_per_gpu_per_step": B, "occ_points_per_scene": M, "grasp_points_per_scene": 1,
                   "parallelism": f"scene-sharded x{world} (scene i -> rank i mod {world}; replicas, no data-path collective)"},
        "step_ms_median": float(np.median(step_ms)), "step_ms_max": float(np.max(step_ms)),
        "query_points_per_sec": scenes_per_s * points_per_scene,
        "algorithmic_tflops": scenes_per_s * flop_scene / 1e12,
        "roofline": {
            "kernel": STAGE_NAMES[dom], "bound": "mfma", "achieved": achieved, "peak": PEAK_F32_MATRIX_TFLOPS,
            "unit": "TFLOP/s", "frac": achieved / PEAK_F32_MATRIX_TFLOPS, "traffic": traffic, "traffic_source": traffic_src,
            "frac_of_measured_peak": achieved / MEASURED_F32_MATRIX_TFLOPS,
            "avg_launch_ms": dom_avg_ms, "median_launch_ms": float(np.median(dom_ms)), "flops_per_launch": dom_flops,
            # the persistent U-Net launch in its default form issues fewer FLOPs than it is credited with (Winograd): the matrix pipe's own load
            "issued_mfma_flops_per_launch": unet_issued_flops(B) if dom == UNET_STAGE else None,
            "issued_mfma_frac_of_peak": unet_issued_flops(B) / (dom_avg_ms * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS if dom == UNET_STAGE else None,
            "note": "fp32-input MFMA (v_mfma_f32_16x16x4_f32 / 32x32x2_f32) peak; `achieved` / `frac` count the ALGORITHMIC direct-convolution FLOPs of SURVEY 8d -- "
                    "the launch runs its 3x3 layers as Winograd F(2x2, 3x3) and ISSUES issued_mfma_flops_per_launch; events on the launch stream inside the timed steps (even steps); "
                    "kernel = the longest launch of the step as it is launched: the persistent U-Net launch (twelve layers, "
                    "algorithmic FLOPs of all of them) when that form is in use, else unet.up0.conv1 unless another stage exceeds "
                    "1.15x its time (pick_headline)",
            # the kernel VERDICT r01 named (roofline_frac 0.46 then), measured the same way on the odd steps
            "r01_kernel": {"kernel": STAGE_NAMES[NAMED_STAGE], "achieved": named_ach, "frac": named_ach / PEAK_F32_MATRIX_TFLOPS,
                           "frac_of_measured_peak": named_ach / MEASURED_F32_MATRIX_TFLOPS, "avg_launch_ms": named_avg_ms,
                           "median_launch_ms": float(np.median(named_ms)), "flops_per_launch": named_flops,
                           "traffic": named_traffic, "traffic_source": named_src},
        },
        "launches_per_step": launches_per_step,
    }
    if stage_ms is not None:
        out["roofline"].update(stage_report(B, M, stage_ms, dec_grasp_ms, dec_occ_ms, unet_ms, persistent_unet, bracket_ms))
        out["stage_note"] = ("unet.conv_final is not launched in this call: the 1x1 convolution is folded into the heads' fc_c weights "
                             "(GIGA_FOLD_FINAL); its entry is the empty event bracket")
    return out


def stage_report(B, M, stage_ms, dec_grasp_ms, dec_occ_ms, unet_ms, persistent_unet, bracket_ms):
    """The untimed pre-pass as roofline keys: time, FLOPs, share of the step and fraction of the fp32-MFMA peak of every stage,
    the U-Net launch, the argmax and worst stage and the FLOP-weighted fraction of the whole step."""
    # shares of the step as it is launched: with the persistent U-Net the twelve layers are one launch of unet_ms
    unet_layers_ms = sum(stage_ms[2:14])
    step_total = sum(stage_ms[:2]) + (unet_ms if persistent_unet else unet_layers_ms) + dec_grasp_ms + dec_occ_ms
    layer_scale = unet_ms / unet_layers_ms if persistent_unet else 1.0     # a layer's share inside the persistent launch, pro rata
    stages = {}
    for i, v in enumerate(stage_ms):
        fl = stage_flops(i, B)
        stages[STAGE_NAMES[i]] = {"ms": round(v, 4), "gflop": round(fl / 1e9, 3),
                                  "share_of_step": round(v * (layer_scale if 2 <= i < 14 else 1.0) / step_total, 3),
                                  "frac_of_fp32_mfma_peak": round(fl / (v * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 3) if fl and v > 0 else None}
    for nm, v, fl in (("decoder.grasp_heads(1 query)", dec_grasp_ms, B * FLOP_GRASP3),
                      ("decoder.occupancy(2048 queries)", dec_occ_ms, B * M * FLOP_HEAD["tsdf"])):
        stages[nm] = {"ms": round(v, 4), "gflop": round(fl / 1e9, 3), "share_of_step": round(v / step_total, 3),
                      "frac_of_fp32_mfma_peak": round(fl / (v * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 3)}
    named = [(k, v) for k, v in stages.items() if v["frac_of_fp32_mfma_peak"] is not None]
    big = [(k, v) for k, v in named if v["share_of_step"] >= 0.08]
    wk, wv = min(big or named, key=lambda kv: kv[1]["frac_of_fp32_mfma_peak"])
    worst_stage = {"kernel": wk, "frac": wv["frac_of_fp32_mfma_peak"], "share_of_step": wv["share_of_step"], "ms": wv["ms"],
                   "note": "lowest fraction of the fp32-MFMA peak among the stages with >= 8 % of the step"}
    ak, av = max(stages.items(), key=lambda kv: kv[1]["ms"])
    argmax_stage = {"kernel": ak, "ms": av["ms"], "frac": av["frac_of_fp32_mfma_peak"]}
    step_flops = sum(v["gflop"] for v in stages.values()) * 1e9
    unet_flops = stage_flops(UNET_STAGE, B)
    unet_launch = {"ms": round(unet_ms, 4), "gflop": round(unet_flops / 1e9, 3), "share_of_step": round(unet_ms / step_total, 3),
                   "frac_of_fp32_mfma_peak": round(unet_flops / (unet_ms * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS, 3),
                   "sum_of_the_twelve_layers_as_separate_launches_ms": round(unet_layers_ms, 4),
                   "form": "one persistent launch (unet_mega_kernel)" if persistent_unet else "one launch per layer"} if unet_ms else None
    if unet_launch and persistent_unet:                       # the launch the step really contains; its twelve layers stay listed beside it
        stages[STAGE_NAMES[UNET_STAGE]] = unet_launch
        argmax_stage = {"kernel": STAGE_NAMES[UNET_STAGE], "ms": unet_launch["ms"], "frac": unet_launch["frac_of_fp32_mfma_peak"]}
    return {
        # elapsed time of an EMPTY event bracket on the same stream: contained in every *_launch_ms / stage ms of the roofline
        # (rocprofv3's kernel durations under profiles/ do not contain it)
        "empty_event_bracket_ms": bracket_ms,
        "unet_launch": unet_launch,
        "stages_note": "the U-Net layers of `stages` are timed as SEPARATE launches (probing one layer switches that call to "
                       "per-layer launches); inside the persistent launch their shares are scaled pro rata",
        "stages": stages,
        # The roofline kernel is the LONGEST launch, which is also the best-tuned one.  Beside it: the true argmax
        # of the measured stage times, the stage FURTHEST below the roofline among those that take >= 8 % of the step,
        # and the FLOP-weighted fraction of the whole step (sum of algorithmic FLOPs / sum of stage times).
        "argmax_stage": argmax_stage, "worst_stage": worst_stage,
        "step_frac_flop_weighted": step_flops / (step_total * 1e-3) / 1e12 / PEAK_F32_MATRIX_TFLOPS,
    }


def bench_c3_gather(net, x, pos, pos_occ, sharding, dist, rccl, rank, world, B, dev):
    """BASELINE config c3: world x B scenes sharded over the ranks, the head outputs of ALL scenes gathered on every rank
    with one RCCL all_gather per output tensor (giga_amd.sharding.all_gather_scenes).  Checks the gathered result against
    this rank's own rows and reports the time of the collective (not part of `value`)."""
    n = world * B
    with torch.no_grad():
        local = net(x, pos, p_tsdf=pos_occ)
        torch.cuda.synchronize()
        full = sharding.all_gather_scenes(tuple(local), n, rank, world, rccl)     # warm-up (communicator setup)
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        full = sharding.all_gather_scenes(tuple(local), n, rank, world, rccl)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    mine = sharding.scene_shard(n, rank, world)
    ok = all(tuple(f.shape[1:]) == tuple(l.shape[1:]) and f.shape[0] == n and torch.equal(f[mine], l)
             for f, l in zip(full, local))
    okt = torch.tensor([1.0 if ok else 0.0], device=dev)
    dist.all_reduce(okt, op=dist.ReduceOp.MIN, group=rccl)
    nbytes = sum(f.numel() * 4 for f in full)
    return {"workload": f"c3: {n} scenes = {B}/GPU x {world}, all_gather of qual/rot/width/occ of every scene over RCCL",
            "scenes": n, "gathered_bytes_per_rank": nbytes, "all_gather_ms": dt * 1e3, "own_rows_match_on_every_rank": bool(okt.item() == 1.0),
            "checksum_qual": float(full[0].double().sum())}


def empty_bracket_ms(L, _capi, dev, reps=15):
    """Elapsed time between two HIP event records with NOTHING between them on the launch stream (median): every HIP-event
    kernel duration in this file contains it, which matters for the 10-50 us kernels (rocprofv3's kernel durations, committed
    under profiles/, do not)."""
    a, b = L.giga_event_create(), L.giga_event_create()
    ms, out = ctypes.c_float(), []
    with torch.cuda.device(dev):
        st = _capi.stream_ptr(dev)
        for _ in range(reps):
            torch.cuda.synchronize()
            L.giga_event_record(a, st); L.giga_event_record(b, st)
            _capi.check(L.giga_event_elapsed_ms(a, b, ctypes.byref(ms)), "event")
            out.append(ms.value)
    L.giga_event_destroy(a); L.giga_event_destroy(b)
    return float(np.median(out))


def _settle():
    """Let the container's CPU quota refill before a timed region.  The build / GPU boxes run under a CFS quota: a leg that has
    just burnt CPU (synthetic scenes, packing) gets its final synchronize() throttled for 40-80 ms -- measured in tools runs as
    a 78-ms synchronize() after 9 ms of GPU work with every per-step GPU interval normal.  Untimed, and always FOLLOWED by the
    warm-up steps: after 0.25 s of idling the GPU runs its first milliseconds at reduced clocks (measured: headline step 0.487
    instead of 0.467 ms when the pause sat between warm-up and timed region)."""
    time.sleep(0.25)


def _rewarm(fn, least, min_ms=30.0):
    """At least `least` untimed calls of fn and at least min_ms of GPU work after a _settle() pause.  With more than one rank
    the count is FIXED (16 calls beyond `least`): fn may contain a collective (the data-parallel training step all-reduces its
    gradients), and a time-based count would differ between ranks."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        for _ in range(max(least, 4) + 16):
            fn()
        torch.cuda.synchronize()
        return
    t0, n = time.perf_counter(), 0
    while n < least or (time.perf_counter() - t0) * 1e3 < min_ms:
        for _ in range(4):
            fn()
        n += 4
        torch.cuda.synchronize()


def _time_steps(fn, steps, warm):
    _settle()                              # (before the warm-up: an idle GPU drops its clocks, the warm-up brings them back)
    _rewarm(fn, max(warm, 3))
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        fn()
    marks[steps].record()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    per = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    return el / steps, per


def bench_c4(net, dev, L, _capi, synth, decode_heads, prec, Bc=32, steps=10):
    """c4: Bc scenes x the 64 000-point inference lattice, three grasp heads, encoder AND decoder in precision `prec`
    ('fp16': f16 operands; 'fp16x3': split-operand f16 MFMA in conv_in, the U-Net and the decoder, fp32-grade results).
    After the timed region the first scene of the step's own output is checked against the CPU oracle."""
    N = 64000
    net.set_precision(prec)
    blob = net.packed_blob(dev)
    from giga_amd.detection import query_lattice
    x = torch.from_numpy(synth.tsdf_batch(1000, Bc)).to(dev)
    lat = query_lattice(40, dev)          # the VGNImplicit lattice (detection_implicit.py:28-31), shared by the batch
    ev = [(L.giga_event_create(), L.giga_event_create()) for _ in range(steps)]

    def step(pr=None):
        with torch.no_grad():
            nhwc, _ = net.encoder.encode_nhwc(x, blob=blob, precision=prec, fold_final=True)
            return decode_heads(nhwc, lat, blob, 7, prec, True, probe=pr, folded=True)

    _settle()
    _rewarm(step, 8)                       # also absorbs the allocator's one-off work after a change of batch size
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        step(ev[i])
    marks[steps].record()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    per_step = [marks[i].elapsed_time(marks[i + 1]) for i in range(steps)]
    ms = ctypes.c_float()
    dms = []
    for a, b in ev:
        _capi.check(L.giga_event_elapsed_ms(a, b, ctypes.byref(ms)), "event")
        dms.append(ms.value)
        L.giga_event_destroy(a); L.giga_event_destroy(b)
    dec_ms = float(np.median(dms))
    checked = check_c4_scene(step(), prec, synth)           # (untimed) this leg's own output, scene 0, against the oracle
    bracket_ms = empty_bracket_ms(L, _capi, dev)
    flops = Bc * N * FLOP_GRASP3
    ach = flops / (dec_ms * 1e-3) / 1e12
    net.set_precision("fp32")
    split = prec == "fp16x3"
    mixed = prec == "fp16x3+fp16"          # f16x3 encoder (fp32 planes) under the plain-f16 lattice decoder
    tr, tr_src = traffic_lookup("c4step_x3" if split else "c4step", "decoder_lat_kernel") if Bc == 32 and not mixed else (None, None)
    kname = "decoder_lat_kernel" if (split or Bc >= 4) else "decoder_f16s_kernel"
    roof = {"kernel": kname, "bound": "mfma", "achieved": ach,
            "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_F16_MFMA_TFLOPS, "traffic": tr, "traffic_source": tr_src,
            "frac_of_measured_peak": ach / MEASURED_F16_MFMA_TFLOPS, "avg_launch_ms": dec_ms, "flops_per_launch": flops,
            # the HIP-event bracket itself (two records with nothing between them); `frac` above is NOT corrected for it
            "empty_event_bracket_ms": bracket_ms,
            "frac_net_of_bracket": flops / (max(dec_ms - bracket_ms, 1e-6) * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS}
    if kname == "decoder_lat_kernel":
        r = ISSUED_PER_ALGORITHMIC["fp16" if mixed else prec]
        roof["issued_mfma_tflops"] = ach * r
        roof["issued_mfma_frac_of_peak"] = ach * r / PEAK_F16_MFMA_TFLOPS
        roof["note"] = ("`achieved`/`frac` count ALGORITHMIC FLOPs (154 560 per point, SURVEY 8d).  The kernel evaluates the xz / xy thirds of "
                        "fc_c, fc_p and the stream's biases once per plane pixel of a (scene, ix) slab instead of once per point and injects "
                        "them through one-hot K = 16 MFMAs: it ISSUES %d f16 MFMAs per 32-point tile and head (%s), i.e. issued_mfma_tflops "
                        "keeps the matrix pipe busy" % ((107, "f16x3: three per operand pair") if split else (43, "58 before")))
    return {
        "workload": f"c4: batch={Bc} scenes x the 64000-point inference lattice, 3 grasp heads, "
                    + ("f16x3 split-operand f16-MFMA encoder and decoder (fp32-grade, <= 6e-6 vs oracle)" if split else
                       "f16x3 split-operand encoder (fp32-grade planes) + plain f16 MFMA decoder (lattice path)" if mixed else
                       "f16 MFMA decoder (lattice path) + f16 encoder"),
        "checked_vs_oracle": checked,
        "scenes_per_sec": Bc * steps / el, "query_points_per_sec": Bc * steps * N / el,
        "ms_per_step": el / steps * 1e3, "step_ms_median": float(np.median(per_step)), "step_ms_max": float(np.max(per_step)),
        "dtype": "f16x3 split operands / f32 accumulate" if split else
                 "encoder f16x3 split operands, decoder f16 operands / f32 accumulate" if mixed else "f16 operands / f32 accumulate",
        "roofline": roof,
    }


def bench_c4_graph(net, dev, synth, decode_heads, prec, Bc=1, replays=300):
    """The c4 network call (encoder + lattice decode of Bc scenes) captured ONCE into a hipGraph and replayed: what a planner loop
    pays per call when the host only replays (giga_amd.detection.VGNImplicit does that), without this file's event brackets and
    without the per-launch host cost of five library calls.  The replayed output is checked against the oracle afterwards."""
    net.set_precision(prec)
    blob = net.packed_blob(dev)
    from giga_amd.detection import query_lattice
    x = torch.from_numpy(synth.tsdf_batch(1000, Bc)).to(dev)
    lat = query_lattice(40, dev)

    def step():
        with torch.no_grad():
            nhwc, _ = net.encoder.encode_nhwc(x, blob=blob, precision=prec, fold_final=True)
            return decode_heads(nhwc, lat, blob, 7, prec, True, folded=True)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    _settle()
    for _ in range(200):
        graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    checked = check_c4_scene(out, prec, synth)
    net.set_precision("fp32")
    return {"workload": f"c4 network call on {Bc} scene(s) x the 64000-point lattice, {prec}, one hipGraph replay per call",
            "ms_per_call": el / replays * 1e3, "scenes_per_sec": Bc * replays / el, "replays": replays, "checked_vs_oracle": checked}


_C4_ORACLE = {}
C4_TOL = {"fp32": 1e-4, "fp16x3": 1e-4, "fp16": 1e-2, "fp16x3+fp16": 5e-3}       # the tolerances of tests/test_gpu_c4_shapes.py (rot, width: x2)


def check_c4_scene(out, prec, synth):
    """The oracle as the CHECKER of what the c4 legs time: scene 0 of the batch (synthetic scene 1000) on the 64 000-point
    lattice, qual / rot / width of the step's own output against `O.model_forward`.  Raises if out of tolerance."""
    from oracle import giga_oracle as O
    from giga_amd import weights
    if "ref" not in _C4_ORACLE:
        with torch.no_grad():
            _C4_ORACLE["ref"] = O.model_forward(weights.make_state_dict(7), torch.from_numpy(synth.tsdf_batch(1000, 1)),
                                                O.inference_lattice())
    errs = {}
    for name, key, scale in (("qual", "decoder_qual", 1.0), ("rot", "decoder_rot", 2.0), ("width", "decoder_width", 2.0)):
        got = out[key][0:1].float().cpu()
        e = float((got - _C4_ORACLE["ref"][("qual", "rot", "width").index(name)]).abs().max())
        errs[name] = e
        if not e < C4_TOL[prec] * scale:
            raise AssertionError(f"c4 {prec}: {name} of scene 0 is {e:.3e} off the oracle (tolerance {C4_TOL[prec] * scale:.0e})")
    return {"scene": 1000, "points": 64000, "max_abs_err": errs, "tolerance": C4_TOL[prec]}


def check_c2_scene(out, sd, x, pos, pos_occ):
    """The oracle as the CHECKER of the headline step (c2, strict fp32): the first scene of this rank's batch, its single grasp query
    (qual, rot, width) and its 2048 occupancy logits, against `O.model_forward` (conv_onet/models/__init__.py:42-67 restated) at the
    fp32 tolerance of tests/test_gpu_parity.py.  Raises if out of tolerance."""
    from oracle import giga_oracle as O
    with torch.no_grad():
        ref = O.model_forward(sd, x[0:1].cpu(), pos[0:1].cpu(), p_tsdf=pos_occ[0:1].cpu())
    errs = {}
    for name, got, want, tol in zip(("qual", "rot", "width", "tsdf"), out, ref, (1e-4, 2e-4, 2e-4, 2e-4)):
        e = float((got[0:1].float().cpu() - want).abs().max())
        errs[name] = e
        if not e < tol:
            raise AssertionError(f"c2 fp32: {name} of scene 0 is {e:.3e} off the oracle (tolerance {tol:.0e})")
    return {"scene": "first scene of rank 0's shard", "max_abs_err": errs, "tolerance": 1e-4}


def bench_c4_generic(net, dev, L, _capi, synth, decode_heads, prec, Bc=32, steps=8):
    """c4 with ARBITRARY query points: 64 000 random queries per scene (each scene its own set) instead of the 40^3 inference lattice,
    i.e. LocalDecoder.forward with a general `p` (decoder.py:133-176): bilinear gathers from the planes, no separable-fc_c shortcut.
    The decoder here is `decoder_f16_kernel` (fp16: shared-feature kernel) / `decoder_f16s_kernel` (fp16x3: head-resident), the
    kernels the lattice legs do NOT time.  Scene 0 of the step's own output is checked against the oracle afterwards."""
    N = 64000
    net.set_precision(prec)
    blob = net.packed_blob(dev)
    x = torch.from_numpy(synth.tsdf_batch(1000, Bc)).to(dev)
    p = torch.from_numpy(synth.query_points(1000, Bc, N, stream=5)).to(dev)
    ev = [(L.giga_event_create(), L.giga_event_create()) for _ in range(steps)]

    def step(pr=None):
        with torch.no_grad():
            nhwc, _ = net.encoder.encode_nhwc(x, blob=blob, precision=prec, fold_final=True)
            return decode_heads(nhwc, p, blob, 7, prec, True, probe=pr, folded=True)

    _settle()
    _rewarm(step, 6)
    t0 = time.perf_counter()
    for i in range(steps):
        step(ev[i])
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    ms = ctypes.c_float()
    dms = []
    for a, b in ev:
        _capi.check(L.giga_event_elapsed_ms(a, b, ctypes.byref(ms)), "event")
        dms.append(ms.value)
        L.giga_event_destroy(a); L.giga_event_destroy(b)
    dec_ms = float(np.median(dms))
    out = step()
    from oracle import giga_oracle as O
    from giga_amd import weights
    with torch.no_grad():
        ref = O.model_forward(weights.make_state_dict(7), x[0:1].cpu(), p[0:1].cpu())
    errs = {}
    for name, key, want, scale in zip(("qual", "rot", "width"), ("decoder_qual", "decoder_rot", "decoder_width"), ref, (1.0, 2.0, 2.0)):
        e = float((out[key][0:1].float().cpu() - want).abs().max())
        errs[name] = e
        if not e < C4_TOL[prec] * scale:
            raise AssertionError(f"c4 generic {prec}: {name} of scene 0 is {e:.3e} off the oracle (tolerance {C4_TOL[prec] * scale:.0e})")
    net.set_precision("fp32")
    flops = Bc * N * FLOP_GRASP3
    ach = flops / (dec_ms * 1e-3) / 1e12
    split = prec == "fp16x3"
    return {"workload": f"c4 with arbitrary queries: batch={Bc} scenes x 64000 random query points each, 3 grasp heads, {prec}",
            "checked_vs_oracle": {"scene": 1000, "points": N, "max_abs_err": errs, "tolerance": C4_TOL[prec]},
            "within_1e-3_contract": split,
            "scenes_per_sec": Bc * steps / el, "query_points_per_sec": Bc * steps * N / el, "ms_per_step": el / steps * 1e3,
            "roofline": {"kernel": "decoder_f16s_kernel" if split else "decoder_f16_kernel", "bound": "mfma", "achieved": ach,
                         "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_F16_MFMA_TFLOPS, "traffic": None,
                         "avg_launch_ms": dec_ms, "flops_per_launch": flops,
                         "issued_mfma_frac_of_peak": ach * (162.0 / 58.0 if split else 1.0) / PEAK_F16_MFMA_TFLOPS,
                         "note": "generic gather path: 58 f16 MFMAs per 32-point tile and head (162 in the split mode: three per operand pair)"}}


def bench_c4_all(net, dev, L, _capi, synth, decode_heads):
    out = {}
    # for comparison: the same legs with one launch per U-Net layer (GIGA_LAYERWISE_UNET) instead of the default persistent launch
    net.set_persistent_unet("layers")
    for prec, key in (("fp16", "c4_layerwise_unet"), ("fp16x3", "c4_fp16x3_layerwise_unet")):
        r = bench_c4(net, dev, L, _capi, synth, decode_heads, prec)
        out[key] = {k: r[k] for k in ("workload", "scenes_per_sec", "ms_per_step", "step_ms_median", "step_ms_max")}
        out[key]["workload"] += "; one launch per U-Net layer (GIGA_LAYERWISE_UNET)"
    net.set_persistent_unet(False)
    for prec, key in (("fp16", "c4"), ("fp16x3", "c4_fp16x3")):
        out[key] = bench_c4(net, dev, L, _capi, synth, decode_heads, prec)
        sweep = []
        for bc in (1, 8, 128):           # BASELINE c4 is a sweep over the scenes per GPU
            r = bench_c4(net, dev, L, _capi, synth, decode_heads, prec, Bc=bc, steps=10)
            sweep.append({"scenes": bc, "scenes_per_sec": r["scenes_per_sec"], "ms_per_step": r["ms_per_step"],
                          "decoder_ms": r["roofline"]["avg_launch_ms"], "decoder_tflops": r["roofline"]["achieved"],
                          "decoder_frac_of_f16_mfma_peak": r["roofline"]["frac"],
                          "empty_event_bracket_ms": r["roofline"]["empty_event_bracket_ms"],
                          "decoder_frac_net_of_bracket": r["roofline"]["frac_net_of_bracket"],
                          "checked_vs_oracle_max_abs_err": r["checked_vs_oracle"]["max_abs_err"]})
        out[key + "_sweep"] = sweep
        out[key + "_single_scene_graph_replay"] = bench_c4_graph(net, dev, synth, decode_heads, prec)
        out[key + "_generic_queries"] = bench_c4_generic(net, dev, L, _capi, synth, decode_heads, prec)
    # the mixed mode: the f16x3 encoder (fp32-grade planes) under the plain-f16 lattice decoder -- the throughput decoder without
    # plain f16's encoder error.  Its errors against the oracle are the f16 decoder's own floor (tests/test_f16_error_budget.py)
    out["c4_mixed"] = bench_c4(net, dev, L, _capi, synth, decode_heads, "fp16x3+fp16")
    out["c4_mixed"]["within_1e-3_contract"] = all(v < 1e-3 for v in out["c4_mixed"]["checked_vs_oracle"]["max_abs_err"].values())
    # Which of the two c4 modes is inside the north star's 1e-3: ONLY the split mode.  Plain f16 (`c4`) is a throughput mode: its
    # head outputs are 1e-3 ... 1e-2 off the fp32 reference (11-bit operands in encoder and decoder; tests/test_f16_error_budget.py),
    # so the >= 40 % of MFMA peak it reaches is not a contract-grade figure; `c4_fp16x3` (<= 1e-5) is.
    out["c4"]["within_1e-3_contract"] = False
    out["c4_fp16x3"]["within_1e-3_contract"] = True
    out["c4_contract_note"] = ("c4 (plain f16): decoder %.3f of the f16 MFMA peak, NOT within the 1e-3 contract (max errors vs oracle %s); "
                               "c4_fp16x3: %.3f algorithmic (%.3f issued), within the contract (max errors %s)" % (
                                   out["c4"]["roofline"]["frac"], out["c4"]["checked_vs_oracle"]["max_abs_err"],
                                   out["c4_fp16x3"]["roofline"]["frac"], out["c4_fp16x3"]["roofline"].get("issued_mfma_frac_of_peak", 0.0),
                                   out["c4_fp16x3"]["checked_vs_oracle"]["max_abs_err"]))
    return out


def bench_c2_ii(net, dev, synth, B, steps=20):
    """BASELINE c2 (ii): every scene gets 2048 grasp queries (3 heads) and 2048 occupancy queries; fp32 and fp16x3."""
    N = 2048
    x = torch.from_numpy(synth.tsdf_batch(3000, B)).to(dev)
    p = torch.from_numpy(synth.query_points(3000, B, N, stream=2)).to(dev)
    po = torch.from_numpy(synth.query_points(3000, B, N, stream=3)).to(dev)
    flop_scene = FLOP_ENCODER + N * (FLOP_GRASP3 + FLOP_HEAD["tsdf"])
    res = {}
    for prec in ("fp32", "fp16x3"):
        net.set_precision(prec).eval()
        with torch.no_grad():
            el, per = _time_steps(lambda: net(x, p, p_tsdf=po), steps, 5)
        res[prec] = {"ms_per_step": el * 1e3, "step_ms_median": float(np.median(per)), "scenes_per_sec": B / el,
                     "query_points_per_sec": B * 2 * N / el, "algorithmic_tflops": B * flop_scene / el / 1e12}
    net.set_precision("fp32")
    res["workload"] = f"c2 (ii): batch={B}, 2048 grasp queries x 3 heads + 2048 occupancy queries per scene"
    return res


def bench_c2_mode(net, x, pos, pos_occ, prec, steps=30):
    """The headline workload (c2, literal train_giga call) in another precision mode, for comparison with `value`."""
    net.set_precision(prec).eval()
    with torch.no_grad():
        el, per = _time_steps(lambda: net(x, pos, p_tsdf=pos_occ), steps, 5)
    net.set_precision("fp32")
    B = x.shape[0]
    return {"workload": f"c2 in mode {prec}: f16x3 split-operand encoder and decoders (fp32-grade results, <= 6e-6 vs the oracle)",
            "ms_per_step": el * 1e3, "step_ms_median": float(np.median(per)), "scenes_per_sec": B / el}


def bench_train(net, dev, synth, B, M, steps=50, rank=0, world=1, sync=None, precision="fp32", flat=True, giga_adam=False):
    """One optimisation step of scripts/train_giga.py:198-211 on this rank's scenes: forward, the fused joint loss
    (giga_amd.training.giga_loss = select + loss_fn of the reference), HIP backward, fused Adam.  world > 1: the backward
    all-reduces (means) the flat gradient bucket over RCCL (net.enable_data_parallel), BASELINE config c5."""
    from giga_amd.training import giga_loss
    net.set_precision("fp32").train().set_train_precision(precision)
    first = 2000 + rank * B
    x = torch.from_numpy(synth.tsdf_batch(first, B)).to(dev)
    pos = torch.from_numpy(synth.query_points(first, B, 1, stream=2)).to(dev)
    pos_occ = torch.from_numpy(synth.query_points(first, B, M, stream=3)).to(dev)
    y = tuple(torch.from_numpy(a).to(dev) for a in synth.train_labels(first, B, M))
    # the reference's optimiser (train_giga.py:49: Adam, lr 2e-4) in torch's fused form (the default per-tensor foreach path
    # costs 6 ms of host time per step for the 164 parameter tensors); flat: over the module's single flat parameter
    # (net.flatten_parameters(): one Adam launch instead of five, no per-step flattening copy, one gradient for autograd)
    if giga_adam:                                        # the same update as one HIP launch over the flat buffer (giga_amd/optim.py)
        from giga_amd.optim import FlatAdam
        opt = FlatAdam(net.flatten_parameters(), lr=2e-4)
    else:
        opt = torch.optim.Adam(net.flatten_parameters() if flat else [q for q in net.parameters() if q.requires_grad], lr=2e-4, fused=True)
    last = {}

    def step():
        opt.zero_grad(set_to_none=True)
        loss, _ = giga_loss(net(x, pos, p_tsdf=pos_occ), y)
        loss.backward()
        opt.step()
        last["loss"] = loss

    for _ in range(5):
        step()
    if sync is not None:
        sync()
    el, per = _time_steps(step, steps, 0)
    if sync is not None:
        sync()
    # ---- what the step is made of (untimed): the library's launches per step and, one launch per extra step, HIP events around
    # EVERY launch of the step on the stream it runs on (giga_launch_probe); the five longest kernels and the step's roofline
    from giga_amd import _capi
    L = _capi.lib()
    torch.cuda.synchronize()
    n0 = L.giga_launch_count()
    step()
    torch.cuda.synchronize()
    n_launch = int(L.giga_launch_count() - n0)
    kernels = []
    if rank == 0 and world == 1:
        ev0, ev1 = L.giga_event_create(), L.giga_event_create()
        ms = ctypes.c_float()
        for i in range(1, n_launch + 1):
            reps, name = [], ""
            for _ in range(3):
                torch.cuda.synchronize()
                L.giga_launch_probe(L.giga_launch_count() + i, ev0, ev1)
                step()
                if L.giga_event_elapsed_ms(ev0, ev1, ctypes.byref(ms)) == 0:
                    reps.append(ms.value)
                name = _kernel_name((L.giga_launch_probe_name() or b"").decode())
            L.giga_launch_probe(0, None, None)
            if reps:
                kernels.append((float(np.median(reps)), i, name))
        L.giga_event_destroy(ev0); L.giga_event_destroy(ev1)
    net.eval().set_train_precision("fp32")
    arith = {"bf16": "bf16 MFMA operands / fp32 accumulate in the U-Net's forward, data-gradient and 3x3 weight-gradient convolutions and in "
                     "the decoder heads (forward, gradient chain and weight gradients in one fused kernel per call); fp32 conv_in, "
                     "ConvTranspose / 1x1 weight gradients, activations in memory, master weights and optimizer",
             "bf16_convs": "bf16 MFMA operands / fp32 accumulate in the U-Net's convolutions only; fp32 decoders",
             "fp32": "fp32"}[precision]
    # algorithmic FLOPs of the step: 3 x the forward of the literal train_giga call (training ~ 3x forward FLOPs)
    step_flop = 3.0 * B * (FLOP_ENCODER + FLOP_GRASP3 + FLOP_HEAD["tsdf"] * M)
    ach = step_flop / el / 1e12
    by_kernel = {}
    for t, i, name in kernels:
        e = by_kernel.setdefault(name, [0.0, 0])
        e[0] += t; e[1] += 1
    top = sorted(by_kernel.items(), key=lambda kv: -kv[1][0])[:5]
    peak = PEAK_F16_MFMA_TFLOPS if precision.startswith("bf16") else PEAK_F32_MATRIX_TFLOPS
    tr5, tr5_src = traffic_c5(precision) if (B == 32 and M == 2048 and precision != "bf16_convs") else (None, None)
    roof = {"bound": "mfma", "achieved": ach, "peak": peak, "unit": "TFLOP/s", "frac": ach / peak,
            "frac_of_fp32_matrix_peak": ach / PEAK_F32_MATRIX_TFLOPS, "frac_of_bf16_mfma_peak": ach / PEAK_F16_MFMA_TFLOPS,
            "flops_per_step": step_flop, "traffic": tr5, "traffic_source": tr5_src,
            "hbm_time_at_peak_ms": round(tr5 / (PEAK_HBM_GBS * 1e9) * 1e3, 4) if tr5 else None,
            "note": "whole step: 3 x the algorithmic forward FLOPs of the literal train_giga call / the wall time of a step; the "
                    "per-kernel times below are HIP events around each launch of the step (giga_launch_probe), medians of three",
            "sum_of_launch_ms": round(sum(t for t, _, _ in kernels), 4) if kernels else None,
            "five_longest_kernels": [{"kernel": k, "ms_per_step": round(v[0], 4), "launches_per_step": v[1]} for k, v in top]}
    if world > 1:
        roof = None
    return {"workload": f"joint GIGA training step (train_giga.py:198-211): B={B} scenes/GPU, 1 grasp query + {M} "
                        f"occupancy queries, forward + fused loss + HIP backward + fused Adam"
                        f"{' (giga_amd.optim.FlatAdam: one launch)' if giga_adam else ''}"
                        f"{' over one flat parameter' if flat else ' over the 164 parameter tensors'}, {arith}, {world} GPU"
                        + (", one RCCL all-reduce of the flat gradient bucket per step" if world > 1 else ""),
            "steps": steps, "ms_per_step": el * 1e3, "step_ms_median": float(np.median(per)), "step_ms_max": float(np.max(per)),
            "step_ms_p90": float(np.percentile(per, 90)), "scenes_per_sec": world * B / el,
            "launches_per_step": n_launch, "roofline": roof,
            "final_loss": float(last["loss"].detach())}


def _kernel_name(mangled):
    """`_ZN4giga13conv16_kernelIfLi2E...` -> `conv16_kernel<...>` (the name without its template arguments): hipKernelNameRefByPtr
    returns the mangled symbol."""
    import re
    m = re.match(r"_ZN4giga(\d+)", mangled) or re.match(r"_Z(\d+)", mangled)
    if not m:
        return mangled
    n = int(m.group(1))
    name = mangled[m.end():m.end() + n]
    return name + ("<...>" if mangled[m.end() + n:m.end() + n + 1] == "I" else "")


def cpu_baseline(sd, synth, M, budget_s=20.0):
    """Time the CPU oracle (oracle/giga_oracle.py, a port of the reference's PyTorch path pinned to
    reference-generated goldens) on a bounded sample of the same workload.  torch's intra-op pool
    collapses when oversubscribed on very wide hosts, so the thread count is calibrated first
    (best of a few candidates on a 2-scene pass) and reported as `cores`."""
    from oracle import giga_oracle as O
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    Bs = 8
    x = torch.from_numpy(synth.tsdf_batch(0, Bs))
    pos = torch.from_numpy(synth.query_points(0, Bs, 1, stream=2))
    pos_occ = torch.from_numpy(synth.query_points(0, Bs, M, stream=3))

    def one(n):
        t0 = time.perf_counter()
        O.model_forward(sd, x[:n], pos[:n], p_tsdf=pos_occ[:n])
        return time.perf_counter() - t0

    with torch.no_grad():
        cands = sorted({c for c in (8, 16, 32, 64, avail) if c <= avail})
        best, best_t = cands[0], None
        for c in cands:
            torch.set_num_threads(c)
            one(2)
            t = min(one(2), one(2))
            if best_t is None or t < best_t:
                best, best_t = c, t
            if t > 3.0:
                break
        torch.set_num_threads(best)
        one(Bs)
        times = []
        t_start = time.perf_counter()
        while len(times) < 10 and (not times or time.perf_counter() - t_start < budget_s):
            times.append(one(Bs))
        # SURVEY 8d also asks for the reference-shaped single-scene cases: c1 (1 scene, 2048 grasp + 2048 occupancy
        # queries) and the c4 shape (1 scene, the 64 000-point lattice, three grasp heads); median of three passes each
        also = {}
        x1 = x[:1]
        p1 = torch.from_numpy(synth.query_points(0, 1, 2048, stream=2))
        lat = torch.from_numpy(synth.inference_lattice())
        for name, fn in (("c1_scene_2048pts_ms", lambda: O.model_forward(sd, x1, p1, p_tsdf=p1)),
                         ("c4_scene_64000pts_ms", lambda: O.model_forward(sd, x1, lat))):
            fn()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
            also[name] = float(np.median(ts)) * 1e3
    med = float(np.median(times))
    return {"value": Bs / med, "unit": "scenes/s", "cores": best, "kind": "port",
            "sample": f"{len(times)} passes of {Bs} scenes (1 grasp query + {M} occupancy queries each), "
                      f"torch {torch.__version__} CPU fp32, median; {best} intra-op threads chosen from "
                      f"{cands} on a host with {avail} usable cores",
            "ms_per_pass": med * 1e3, "also": also}


if __name__ == "__main__":
    main()
