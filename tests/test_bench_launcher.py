"""bench.py's launch contract: `python bench.py --gpus N` starts its own N ranks, WORLD_SIZE must equal --gpus, and the
whole N > 1 code path (gloo barriers, RCCL group after the timed region, counter all_gather and, with --full, the c3 output
gather and the data-parallel c5 step) runs under the launcher at world size 1 on a single-GPU box."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_gpus_flag_without_devices_is_refused():
    """No silent single-rank run: asking for more GPUs than are visible is an error (here: none are visible)."""
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("two devices visible: the spawn would succeed")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0
    assert "HIP device" in (r.stderr + r.stdout)


def test_world_size_must_match_gpus_flag():
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "4", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                       env=env, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE" in (r.stderr + r.stdout)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_multi_rank_code_path_at_world_size_one():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29731", BENCH, "--gpus", "1", "--steps", "5", "--warmup", "2", "--full", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=580, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    out = json.loads(line)
    assert out["n_gpus"] == 1 and out["steps"] == 5 and out["value"] > 0
    assert len(line) < 6144                                  # the driver parses ONE line; 31 KB came back as parsed = null in round 5
    assert out["rccl_ranks"] == 1 and len(out["per_rank_seconds"]) == 1
    assert out["c3_gather"]["own_rows_match_on_every_rank"] is True and out["c3_gather"]["scenes"] == 32
    assert out["c5_train_step_fp32_data_parallel"]["ms_per_step"] > 0 and out["c5_train_step_bf16_data_parallel"]["ms_per_step"] > 0
    assert set(out["roofline"]) == {"kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "flops_per_launch"}
    full = json.load(open(os.path.join(ROOT, out["extra_file"])))          # everything else is in the side file
    assert full["roofline"]["kernel"] in full["roofline"]["stages"]
    assert full["extra"]["c3_gather"]["checksum_qual"] == full["extra"]["c3_gather"]["checksum_qual"]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_run_is_the_headline_only(tmp_path):
    """Without --full the run is set-up, warm-up and the timed steps: no oracle check, no CPU baseline, no other configs -- also
    under the launcher, where the RCCL MAX-reduce of the elapsed times still runs."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "MASTER_PORT", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    env["GIGA_BENCH_EXTRA"] = str(tmp_path / "bench_extra.json")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
           "--master-port", "29733", BENCH, "--gpus", "1", "--steps", "5", "--warmup", "2"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=280, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["steps"] == 5 and out["warmup"] == 2 and out["value"] > 0 and out["rccl_ranks"] == 1
    assert set(out["roofline"]) == {"kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "flops_per_launch"}
    for k in ("checked_vs_oracle", "cpu_baseline", "c3_gather", "c5_train_step_fp32_data_parallel", "c5_train_step_bf16_data_parallel"):
        assert k not in out, k
    full = json.load(open(tmp_path / "bench_extra.json"))
    assert set(full["extra"]) == {"rccl_ranks", "per_rank_seconds"}


def test_contract_line_is_small_and_round_trips(tmp_path):
    """bench.py's line assembly on canned numbers (the complete record of the round-5 evidence run, 31 KB): the printed line
    carries the contract keys only, stays under 6 KB and survives json.loads; the complete record goes to the side file."""
    sys.path.insert(0, ROOT)
    import bench
    full = json.loads(open(os.path.join(ROOT, "profiles", "r05", "final", "bench.json")).read().strip().splitlines()[-1])
    full.pop("summary")
    full["summary"] = bench.summary_of(full)
    side = tmp_path / "bench_extra.json"
    text = bench.emit(full, path=str(side))
    assert "\n" not in text and len(text) < bench.LINE_LIMIT == 6144
    line = json.loads(text)
    for k in bench.CONTRACT_KEYS:
        assert k in line, k
    assert list(line)[-1] == "summary"
    assert set(line["roofline"]) == set(bench.ROOFLINE_KEYS) and all(not isinstance(v, (dict, list)) for v in line["roofline"].values())
    assert abs(line["roofline"]["frac"] - line["roofline"]["achieved"] / line["roofline"]["peak"]) < 1e-12
    assert set(line["cpu_baseline"]) == set(bench.CPU_BASELINE_KEYS) and line["cpu_baseline"]["value"] > 0
    assert "extra" not in line and "stages" not in line["roofline"]
    assert line["checked_vs_oracle"]["tolerance"] == 1e-4
    kept = json.load(open(side))
    assert "extra" in kept and "stages" in kept["roofline"]                 # nothing measured is lost
    # N > 1 digest keys survive the slimming
    full["extra"].update({"rccl_ranks": 8, "per_rank_seconds": [0.1] * 8, "c3_gather": {"scenes": 256, "all_gather_ms": 1.0,
                                                                                            "own_rows_match_on_every_rank": True, "checksum_qual": 1.0}})
    line = json.loads(bench.emit(full, path=str(side)))
    assert line["rccl_ranks"] == 8 and len(line["per_rank_seconds"]) == 8 and line["c3_gather"]["scenes"] == 256
    # and a summary that could not fit is shed from its tail, never the contract keys
    full["summary"] = {f"k{i}": "x" * 100 for i in range(100)}
    text = bench.emit(full, path=str(side))
    assert len(text) < bench.LINE_LIMIT and all(k in json.loads(text) for k in bench.CONTRACT_KEYS)


def test_result_without_the_pre_pass(tmp_path):
    """A plain run makes no stage pre-pass (persistent U-Net): core_result builds the contract keys and the roofline from the timed
    steps alone; given the pre-pass's numbers (--full) it adds the table of every stage."""
    import argparse
    sys.path.insert(0, ROOT)
    import bench
    K = 4
    timed = dict(args=argparse.Namespace(warmup=2), world=1, B=32, M=2048, K=K, T=K * 0.34e-3, scenes_per_s=32 / 0.34e-3,
                 dom=bench.UNET_STAGE, dom_ms=[0.23, 0.23], step_ms=[0.34] * K, named_ms=[0.04, 0.04], launches_per_step=5,
                 persistent_unet=True)
    plain = bench.core_result(stage_ms=None, dec_grasp_ms=None, dec_occ_ms=None, bracket_ms=None, unet_ms=None, **timed)
    assert "stages" not in plain["roofline"] and "stage_note" not in plain
    assert abs(plain["ms_per_step"] - 0.34) < 1e-12 and plain["roofline"]["avg_launch_ms"] == 0.23
    line = json.loads(bench.emit(dict(plain, summary=bench.summary_of(plain)), path=str(tmp_path / "plain.json")))
    assert all(k in line for k in bench.CONTRACT_KEYS) and set(line["roofline"]) == set(bench.ROOFLINE_KEYS)
    full = bench.core_result(stage_ms=[0.04, 0.005] + [0.02] * 12 + [0.006], dec_grasp_ms=0.01, dec_occ_ms=0.05, bracket_ms=0.005,
                             unet_ms=0.23, **timed)
    assert full["roofline"]["stages"][bench.STAGE_NAMES[bench.UNET_STAGE]]["ms"] == 0.23
    assert {k: v for k, v in full["roofline"].items() if k in plain["roofline"]} == plain["roofline"]


def test_dump_outputs_writes_float32_within_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: one float32 .npy per output; beyond the size limit the same fixed sample of scenes is kept of every
    output (and its indices written), identically from call to call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    outs = {"qual": torch.rand(6, 1), "rot": torch.rand(6, 1, 4, dtype=torch.float64), "width": torch.rand(6, 1),
            "tsdf": torch.rand(6, 2048, dtype=torch.float16)}
    bench.dump_outputs(str(tmp_path / "all"), outs)
    for k, v in outs.items():
        a = np.load(tmp_path / "all" / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.float().numpy()), k
    assert not (tmp_path / "all" / "scene_index.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4096 + 2 * (4 + 16 + 4 + 2048 * 4 + 8) + 100)      # room for two scenes
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), outs)
    keep = np.load(tmp_path / "s1" / "scene_index.npy").astype(np.int64)
    assert len(keep) == 2 and np.array_equal(keep, np.load(tmp_path / "s2" / "scene_index.npy"))
    total = 0
    for k, v in outs.items():
        a = np.load(tmp_path / "s1" / f"{k}.npy")
        assert np.array_equal(a, v.float().numpy()[keep]) and np.array_equal(a, np.load(tmp_path / "s2" / f"{k}.npy")), k
        total += os.path.getsize(tmp_path / "s1" / f"{k}.npy")
    assert total + os.path.getsize(tmp_path / "s1" / "scene_index.npy") <= bench.DUMP_LIMIT


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--steps" in r.stderr
