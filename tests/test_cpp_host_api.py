"""The C++ host mirror (include/cilantro_hip/icp.hpp) compiled with g++ against the C ABI."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "test_icp")
BIN2 = os.path.join(ROOT, "tests", "cpp", "bin", "test_model_estimation")


def _ensure_built(hip_lib, orc):
    if not (os.path.exists(BIN) and os.path.exists(BIN2)):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])


def test_cpp_header_compiles_and_fails_loudly_without_device(hip_lib, orc):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])   # compile check of the header
    for b in (BIN, BIN2):
        out = subprocess.run([b, "--expect-no-device"], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_host_api_parity_on_gpu(hip_lib, orc):
    _ensure_built(hip_lib, orc)
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_model_estimation_mirrors_on_gpu(hip_lib, orc):
    """PlaneRANSACEstimator3f / KMeans3f through include/cilantro_hip/model_estimation.hpp"""
    _ensure_built(hip_lib, orc)
    out = subprocess.run([BIN2], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_solve_fast_paths_on_host(hip_lib, orc):
    """cilantro_amd/csrc/solve.hpp is shared by the host API and the single-lane device epilogue: its fast paths (polar
    iteration for the rotation() polish, unpivoted register-resident LDL^T) against the general ones (SVD, pivoted LDL^T
    with pseudo-inverse), compiled for the host -- no GPU needed."""
    binp = os.path.join(ROOT, "tests", "cpp", "bin", "test_solve")
    if not os.path.exists(binp):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    out = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_loop_policy_on_host(hip_lib, orc):
    """cilantro_amd/csrc/loop_policy.hpp decides the kernel form of every ICP iteration (cilhip_icp_run and the sharded runs
    share it): its integer and strict-inequality rules at their boundaries, compiled with the host compiler -- no GPU needed."""
    binp = os.path.join(ROOT, "tests", "cpp", "bin", "test_loop_policy")
    if not os.path.exists(binp):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    out = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_grid_policy_on_host(hip_lib, orc):
    """cilantro_amd/csrc/grid_policy.hpp shapes the grid of every search (build_grid): on boxes at the edges of the f32 range,
    degenerate, inverted, infinite and NaN it returns within a bounded number of growth steps, keeps the dimension caps, leaves
    finite normal f32 parameters and puts every coordinate of the box into a data cell -- or refuses; compiled with the host
    compiler, no GPU needed."""
    binp = os.path.join(ROOT, "tests", "cpp", "bin", "test_grid_policy")
    if not os.path.exists(binp):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    out = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_device_mem_on_host(hip_lib, orc):
    """cilantro_amd/csrc/device_mem.hpp owns every device allocation of the library: its owners (single buffer, shared buffer,
    per-call pool) over a counting allocator backed by malloc that can fail a chosen request -- growth, failure, moves, every
    release order of three sharers, early returns; live count and bytes back at their start after each case.  Host compiler, no GPU."""
    binp = os.path.join(ROOT, "tests", "cpp", "bin", "test_device_mem")
    if not os.path.exists(binp):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    out = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_ransac_sampling_on_host(hip_lib, orc):
    """cilantro_amd/csrc/ransac_sampling.hpp draws the samples of both RANSAC estimators and checks a caller's: bit for bit against
    a literal copy of the loop the two estimator files used to carry, over cloud sizes 1 .. 0xFFFFFFF0, a few hundred seeds and 1, 7
    and 128 iterations -- distinct indices below n, zeros behind a short sample, exactly the arrays with an index in use >= n
    refused.  Host compiler, no GPU."""
    binp = os.path.join(ROOT, "tests", "cpp", "bin", "test_ransac_sampling")
    if not os.path.exists(binp):
        subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    out = subprocess.run([binp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
