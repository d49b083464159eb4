"""CPU: the C++ mirror of the image conversions (include/cilantro_hip/image_point_cloud_conversions.hpp, PointCloud3f::fromDepthImage /
fromRGBDImages) and the example compile against the public headers and the library; what needs no device runs."""
import os
import subprocess

from test_components_refs_cpu import ROOT, build_cpp

HERE = os.path.dirname(os.path.abspath(__file__))


def test_cpp_mirror_and_example_compile():
    exe = build_cpp(os.path.join(HERE, "cpp", "test_image_conversions.cpp"), "test_image_conversions")
    build_cpp(os.path.join(ROOT, "examples", "depth_image_conversions.cpp"), "example_depth_image_conversions")
    build_cpp(os.path.join(ROOT, "examples", "projective_icp.cpp"), "example_projective_icp")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
