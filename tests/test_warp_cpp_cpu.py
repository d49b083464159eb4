"""CPU: the warp-field classes of cilantro_hip/icp.hpp and PointCloud3f::transformed(TransformSet) compile on the host against the
library, with examples/non_rigid_icp.cpp; the host half of the mirror runs without a device.  (GPU: the same program's `run` mode.)"""
import os
import subprocess

import pytest

from test_components_refs_cpu import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mirror_and_example_compile():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_warp_field.cpp"), "test_warp_field")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    example = build_cpp(os.path.join(ROOT, "examples", "non_rigid_icp.cpp"), "example_non_rigid_icp")
    r = subprocess.run([example], capture_output=True, text=True)
    assert r.returncode == 0 and "PLY" in r.stdout


@pytest.mark.gpu
def test_cpp_mirror_registers_a_bent_surface():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_warp_field.cpp"), "test_warp_field")
    r = subprocess.run([exe, "run"], capture_output=True, text=True)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
