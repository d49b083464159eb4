"""CPU: the affine warp-field classes of cilantro_hip/icp.hpp, SimpleCombinedMetricDenseRigidWarpFieldICP3f and
resampleAffineTransforms compile on the host against the library; the host half of the mirror runs without a device.  (GPU: the same
program's `run` mode, from tests/test_gpu_warp_field_affine.py.)"""
import os
import subprocess

from test_components_refs_cpu import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_compiles_and_its_host_half_runs():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_warp_field_affine.cpp"), "test_warp_field_affine")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
