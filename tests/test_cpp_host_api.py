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


def test_option_table_sweep_on_host(hip_lib, orc):
    """cilantro_amd/csrc/ctx_options.hpp holds every context option once (fields, default, range, how a value is stored, what it makes
    stale); cilhip_set_option / cilhip_get_option work on a context constructed on the host.  tests/cpp/test_ctx_options.cpp sets every
    row to {default, min, max, min - 1, max + 1, midpoint, 0.5, 1.5, 2.5, 3, 5, 16, 1e-10, NaN}, by key and by id, plus keys and ids the
    table does not hold, each on a fresh context with a stored set of every kind, and prints return code, the read-back of all options
    (as what differs from a fresh context's, which the first line holds in full), the four stored-set flags and the error text, the
    two ways of setting on one line where they agree in everything: byte for byte tests/golden/option_sweep.txt, recorded from the same program against
    the library as it was before the table moved -- once plainly, once under the address and undefined-behaviour sanitizers.  No GPU."""
    want = open(os.path.join(ROOT, "tests", "golden", "option_sweep.txt"), "rb").read()
    lines = want.decode().splitlines()
    from cilantro_amd import capi

    keys = [o["key"] for o in capi.options()]
    # what "accepted keys" means, by behaviour: every table key takes its default, a key absent from the table is refused
    for k in keys:
        first = next(ln for ln in lines if ln.startswith("key+id %s = " % k))      # (the first value of a row is its default)
        assert "-> rc 0 | - |" in first and first.endswith("| "), first
    assert lines[0].startswith("fresh ") and [kv.split("=")[0] for kv in lines[0].split()[1:]] == keys
    assert any(ln.startswith("key no_such_option = 1 -> rc -1 |") and ln.endswith("set_option: unknown key") for ln in lines)
    assert len(lines) == 14 * len(keys) + 4 and sum("-> rc -1 |" in ln for ln in lines) > 150
    for name in ("test_ctx_options", "test_ctx_options_san"):
        binp = os.path.join(ROOT, "tests", "cpp", "bin", name)
        if not os.path.exists(binp):
            subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
        out = subprocess.run([binp], capture_output=True, timeout=120)
        assert out.returncode == 0 and not out.stderr, out.stderr[-2000:]
        assert out.stdout == want, name
