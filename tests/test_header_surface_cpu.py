"""CPU: the C++ headers' shared plumbing (include/cilantro_hip/abi.hpp).  tests/cpp/test_header_surface.cpp pins the public surface of the
classes that sit on shared bases with static_asserts -- it compiling is that check --, then runs the refusals that never reach the library
and, on a machine without a device, every wrapper that turns a return code into an exception."""
import os
import re
import subprocess

import pytest

from test_components_refs_cpu import ROOT, build_cpp

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(ROOT, "include", "cilantro_hip")


@pytest.fixture(scope="module")
def exe():
    """the program, built once: that it compiles is the check of the static_asserts"""
    return build_cpp(os.path.join(HERE, "cpp", "test_header_surface.cpp"), "test_header_surface")


def test_surface_compiles_and_host_refusals_keep_their_texts(exe):
    r = subprocess.run([exe, "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr


def test_every_wrapper_reports_the_failing_entry_and_its_own_text(exe):
    """the table is the one of a machine without a device, so the child sees none, whatever this machine has"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    r = subprocess.run([exe, "nodevice"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "nodevice OK" in r.stdout, r.stdout + r.stderr


def test_headers_under_wall_werror():
    """the headers, through the program that includes all of them that cross the C ABI, give no warning"""
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "cpp", "test_header_surface.cpp")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


def test_include_graph():
    text = {f: open(os.path.join(INCLUDE, f)).read() for f in os.listdir(INCLUDE) if f.endswith(".hpp")}
    # abi.hpp stands on c_api.h and the standard library alone
    assert re.findall(r'#include "([^"]+)"', text["abi.hpp"]) == ["c_api.h"]
    # no header dropped an include it had: icp.hpp brings abi.hpp, the others keep including icp.hpp
    assert '#include "abi.hpp"' in text["icp.hpp"]
    for f in ("clustering.hpp", "kd_tree.hpp", "normal_estimation.hpp", "model_estimation.hpp", "fusion.hpp", "grid_downsampler.hpp", "image_point_cloud_conversions.hpp"):
        assert '#include "icp.hpp"' in text[f], f
    assert '#include "clustering.hpp"' in text["kd_tree.hpp"]
