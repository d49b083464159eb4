"""GPU: the C++ classes that sit on shared bases (include/cilantro_hip/: clustering, kd-trees, normal estimators, RANSAC estimators) against
a direct call of their C entries -- the headers only marshal, so every output agrees bit for bit.  One build and one run of
tests/cpp/test_header_parity.cpp, which states the shapes."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_every_wrapper_returns_the_bits_of_its_entry():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_header_parity.cpp"), "test_header_parity")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "parity OK" in r.stdout, r.stdout[-4000:] + r.stderr[-2000:]
    assert "UNREPEATABLE" not in r.stdout, r.stdout[-4000:]
