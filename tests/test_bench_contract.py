"""bench.py's --gpus contract: the flag is a claim the run has to earn -- the script spawns its own ranks when no
torchrun environment is present, refuses when the GPUs do not exist, and computes `value` / `n_gpus` from what the ranks report.
No reference line: the reference has no benchmark and no multi-GPU path."""
import importlib
import json
import os
import subprocess
import sys
import time

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def bench(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2V_BENCH_ONE_DEVICE", "S2V_BENCH_BACKEND"):
        monkeypatch.delenv(k, raising=False)
    sys.path.insert(0, ROOT)
    try:
        yield importlib.import_module("bench")
    finally:
        sys.path.remove(ROOT)


@pytest.mark.skipif(torch.cuda.is_available(), reason="the no-GPU refusal")
def test_gpus_2_without_gpus_or_env_refuses(bench):
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "2"])
    assert e.value.code not in (0, None)
    assert "no GPU visible" in str(e.value.code)


def test_flag_and_world_size_must_agree(bench, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "8"])
    assert "WORLD_SIZE=1" in str(e.value.code)
    monkeypatch.setenv("WORLD_SIZE", "4")
    with pytest.raises(SystemExit) as e:
        bench.main(["--gpus", "1"])
    assert "WORLD_SIZE=4" in str(e.value.code)
    with pytest.raises(SystemExit):
        bench.main(["--gpus", "0"])


def test_steps_must_be_a_real_count(bench):
    """ms_per_step divides by --steps: a run with no timed step is refused before anything starts"""
    for argv in (["--steps", "0"], ["--steps", "-1"], ["--steps", "3", "--warmup", "-1"]):
        with pytest.raises(SystemExit) as e:
            bench.main(argv)
        assert "--steps must be >= 1" in str(e.value.code)


def test_plain_run_leaves_everything_beside_the_headline_to_full(bench):
    """without --full a run skips the other launch mode, the roofline passes (and with them the CFG-parallel projection), the video and the
    CPU baseline; --full runs them all, and the --no-* / --single-mode flags still switch single parts off inside it"""
    a = bench.parse_args(["--steps", "3", "--warmup", "1"])
    assert not a.full and a.single_mode and a.no_roofline and a.no_vae and a.no_cpu_baseline
    a = bench.parse_args(["--full"])
    assert a.full and not (a.single_mode or a.no_roofline or a.no_vae or a.no_cpu_baseline)
    a = bench.parse_args(["--full", "--no-vae", "--single-mode"])
    assert a.no_vae and a.single_mode and not (a.no_roofline or a.no_cpu_baseline)


def test_value_is_never_the_flag_times_anything():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "args.gpus *" not in src and "* args.gpus" not in src
    assert '"n_gpus": args.gpus' not in src


def test_pmc_pass_follows_the_workload(bench):
    """the fp8 profile used to be picked for the bf16 line ('_' < 'f')"""
    b, files = bench.pmc_traffic_bytes("attention", "cogvideox-5b-49x480x720")
    assert files and all("fp8" not in f and "_c1_" not in f for f in files), files
    assert b is not None and 1.0e9 < b < 4.0e9
    b8, files8 = bench.pmc_traffic_bytes("attention", "cogvideox-5b-fp8-49x480x720")
    assert files8 and all("fp8" in f for f in files8), files8
    assert bench.pmc_traffic_bytes("attention", "cogvideox-5b-49x720x1280") == (None, [])


@pytest.mark.gpu
def test_gpus_2_on_a_one_gpu_box_refuses():
    if torch.cuda.device_count() >= 2:
        pytest.skip("needs a one-GPU box")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2V_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "n_gpus" not in r.stdout
    assert "only 1 GPU(s) visible" in r.stderr


@pytest.mark.gpu
def test_self_spawned_ranks_report_the_devices_they_ran_on():
    """two self-spawned ranks sharing cuda:0 (gloo: RCCL rejects two ranks on one device): the line counts ONE GPU and two ranks,
    and value = the two ranks' steps over the slower rank's time"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(S2V_BENCH_ONE_DEVICE="1", S2V_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload",
                        "cogvideox-2b-9x256x256", "--no-vae", "--no-roofline", "--no-cpu-baseline", "--single-mode"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["config"]["rccl_ranks"] == 2 and line["config"]["backend"] == "gloo"
    assert line["config"]["launcher"] == "self-spawned" and len(line["config"]["ranks"]) == 2
    assert abs(line["value"] - 2 * line["steps"] / (line["ms_per_step"] * line["steps"] / 1e3)) <= 0.02 * line["value"]
    assert line["config"]["weight_broadcast_gb"] > 0 and line["config"]["outputs_finite"]


def test_cfg_parallel_needs_an_even_number_of_ranks(bench):
    """--cfg-parallel pairs the ranks up (dist.cfg_pair_layout): an odd or single-rank request is refused before anything is launched"""
    for n in ("1", "3"):
        with pytest.raises(SystemExit) as e:
            bench.main(["--gpus", n, "--cfg-parallel"])
        assert "even" in str(e.value.code)


@pytest.mark.gpu
def test_cfg_parallel_pair_on_one_device_reports_video_steps():
    """two self-spawned ranks of ONE CFG-parallel pair sharing cuda:0 (gloo carries the all-gather): the line counts video steps -- each step
    is done by BOTH ranks, so value = steps / time, not 2 x --, names the exchange, and the latents stayed finite on both ranks"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(S2V_BENCH_ONE_DEVICE="1", S2V_BENCH_BACKEND="gloo")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--cfg-parallel", "--steps", "3", "--warmup", "1", "--workload",
                        "cogvideox-2b-9x256x256", "--no-roofline", "--single-mode"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    cfg = line["config"]
    assert line["n_gpus"] == 1 and cfg["rccl_ranks"] == 2 and cfg["samples_per_gpu_per_step"] == 1
    assert cfg["parallelism"] == "cfg-parallel pairs x1" and cfg["cfg_parallel"]["pairs"] == 1 and "all_gather" in cfg["cfg_parallel"]["exchange"]
    assert abs(line["value"] - line["steps"] / (line["ms_per_step"] * line["steps"] / 1e3)) <= 0.02 * line["value"]
    assert cfg["outputs_finite"] and line["scaling"] == "strong"


@pytest.mark.gpu
def test_batch_1_reports_the_half_step_as_the_projection():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2V_BENCH_ONE_DEVICE")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--batch", "1", "--steps", "3", "--warmup", "1", "--workload",
                        "cogvideox-2b-9x256x256", "--full", "--no-roofline", "--single-mode"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["config"]["samples_per_gpu_per_step"] == 1 and line["config"]["projected_cfg_parallel_ms"] == line["ms_per_step"]
    assert abs(line["value"] - 0.5e3 / line["ms_per_step"]) <= 0.02 * line["value"]   # half a step per GPU-step: two GPUs make one step
    assert "cpu_baseline" not in line and line["wall_clock_per_video"] is None


def _bench_line(args, timeout):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "S2V_BENCH_ONE_DEVICE")}
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]), wall


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_little_else():
    """the flagship workload without --full: the headline fields, none of the extras, and at most 30 s of the process outside its steps"""
    line, wall = _bench_line(["--gpus", "1", "--steps", "2", "--warmup", "1"], 600)
    assert line["metric"].startswith("denoise steps/sec (CogVideoX-5B") and line["unit"] == "steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 2 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 0.02 * line["value"]
    cfg = line["config"]
    assert cfg["full"] is False and cfg["outputs_finite"] and cfg["eager_ms_per_step"] is None and cfg["cfg_parallel_projection"] is None
    assert line["roofline"] is None and line["wall_clock_per_video"] is None and "cpu_baseline" not in line
    outside = wall - (line["steps"] + line["warmup"]) * line["ms_per_step"] / 1e3
    print(f"MEASURED plain run: {wall:.1f} s wall, {outside:.1f} s outside the steps")
    assert outside <= 30.0, outside


@pytest.mark.gpu
def test_full_run_still_measures_the_extras():
    """--full on the configs[0] geometry: the other launch mode, the roofline with its per-kernel table, the CFG-parallel projection, the
    video and the CPU baseline are all in the line"""
    line, _ = _bench_line(["--steps", "2", "--warmup", "1", "--workload", "cogvideox-2b-9x256x256", "--full"], 900)
    cfg = line["config"]
    assert cfg["full"] is True and cfg["eager_ms_per_step"] > 0 and cfg["cfg_parallel_projection"]["b1_step_ms"] > 0
    assert "attention" in line["roofline"]["per_kernel"] and line["roofline"]["calibrated_peak"] > 0
    assert line["wall_clock_per_video"]["s_per_video_measured"] > 0 and line["wall_clock_per_video"]["frames_finite"]
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["vae_decode"]["value"] > 0
