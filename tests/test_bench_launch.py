"""bench.py's launch contract (CPU): `python bench.py --gpus N` starts N ranks itself or fails loudly -- it never prints a
1-GPU line for an N-GPU request (round-2 VERDICT, missing 1).  And (GPU) what --dump-outputs writes and what a plain run leaves
to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return e


def test_more_ranks_than_devices_exits_non_zero():
    import torch

    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        pytest.skip("two devices are present")
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300, env=_env())
    assert out.returncode != 0
    assert "HIP device(s) visible" in (out.stdout + out.stderr) and "{" not in out.stdout      # a clear message, no JSON line


def test_world_size_must_match_the_request():
    e = _env()
    e.update({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=300, env=e)
    assert out.returncode != 0 and "WORLD_SIZE = 1" in (out.stdout + out.stderr)


def test_self_launch_spawns_one_rank_per_requested_gpu():
    """the same relaunch path the GPU run takes (torch.distributed.run on 127.0.0.1), with gloo and no device work"""
    out = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--selftest-spawn"], capture_output=True, text=True, timeout=300, env=_env())
    assert out.returncode == 0, out.stdout + out.stderr
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    r = json.loads(line)
    assert r["selftest_spawn"] and r["n_gpus"] == 2 and r["ranks_in_all_reduce"] == 2
    # the per-rank fields an N-rank line carries, gathered over the group by the function bench_icp uses
    assert r["rccl_ranks"] == 2
    assert r["kernel_ms_per_step_per_rank"] == pytest.approx([0.1, 0.2])
    assert r["allreduce_us_per_iteration"] == pytest.approx(20.0) and r["allreduce_us_per_iteration_per_rank"] == pytest.approx([10.0, 20.0])
    assert r["host_enqueue_us_per_iteration_per_rank"] == pytest.approx([1.0, 2.0])


@pytest.mark.gpu
def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: float32 / float64 .npy files of what the timed run computed, within 64 MB; --steps sets the timed
    steps; two runs with the same arguments write the same correspondences and transform"""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "200000", "--no-extras", "--no-cpu-baseline"]
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        out = subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, env=_env())
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert r["steps"] == 3 and r["ms_per_step"] > 0.0
        files = sorted(os.listdir(d))
        assert files == ["nn_source_index.npy", "nn_sq_dist.npy", "nn_target_index.npy", "state.npy", "transform.npy"], files
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(v.dtype in (np.float32, np.float64) for v in arrs.values())
        assert sum(v.nbytes for v in arrs.values()) <= 64 << 20
        assert arrs["transform"].shape == (4, 4) and arrs["state"][0] == 3 and arrs["state"][1] == r["last_ncorr"]
        assert len(arrs["nn_target_index"]) == 200000 and (arrs["nn_target_index"] >= 0).sum() == r["last_ncorr"]
        dumps.append(arrs)
    a, b = dumps
    for k in ("nn_source_index", "nn_target_index", "nn_sq_dist", "state"):
        assert np.array_equal(a[k], b[k]), k
    assert np.allclose(a["transform"], b["transform"], rtol=0.0, atol=1e-6)


@pytest.mark.gpu
def test_plain_run_leaves_the_runs_of_their_own_to_full():
    """A plain run prints the headline line and no figure that takes a run of its own; --full adds them after the same timed steps"""
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--n", "200000"]
    lines = []
    for extra in ([], ["--full"]):
        out = subprocess.run([sys.executable, BENCH] + args + extra, capture_output=True, text=True, timeout=600, env=_env())
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]))
    plain, full = lines
    for r in (plain, full):
        assert r["unit"] == "pairs/s" and r["higher_is_better"] and r["dtype"] == "f32 search / f64 accumulate+solve"
        assert r["steps"] == 3 and r["ms_per_step"] > 0.0 and r["value"] == pytest.approx(200000 * 1e3 / r["ms_per_step"])
    runs_of_their_own = ("icp_estimate_ms_15iter_cold", "without_warm_start", "converging_run", "independent_source", "variants",
                         "multi_device_c_loop_one_shard", "cpu_baseline")
    assert [k for k in runs_of_their_own if k in plain] == [] and plain["roofline"]["measured_copy_bandwidth_GBps"] is None
    assert [k for k in runs_of_their_own if k not in full or (isinstance(full[k], dict) and "error" in full[k])] == []
    assert full["roofline"]["measured_copy_bandwidth_GBps"] > 0.0 and full["cpu_baseline"]["value"] > 0.0
