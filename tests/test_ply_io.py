"""PLY ingest / output either side of the path: the Python reader / writer, the C++ header
(include/cilantro_hip/point_cloud.hpp) and their interoperability.  CPU only."""
import os
import subprocess

import numpy as np
import pytest

from cilantro_amd.ply_io import read_ply, write_ply

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "bin", "test_ply")


def _cloud(n=500, seed=0):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(n, 3)).astype(np.float32)
    nr = rng.normal(size=(n, 3)).astype(np.float32); nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    c = (rng.integers(0, 256, (n, 3)) / 255.0).astype(np.float32)
    return p, nr, c


@pytest.mark.parametrize("binary", [True, False])
def test_python_round_trip(tmp_path, binary):
    p, nr, c = _cloud()
    f = str(tmp_path / "a.ply")
    write_ply(f, p, nr, c, binary=binary)
    r = read_ply(f)
    assert np.array_equal(r["points"], p) and np.array_equal(r["normals"], nr)          # %.9g round-trips f32 exactly
    assert np.array_equal(np.round(r["colors"] * 255), np.round(c * 255))
    write_ply(f, p, binary=binary)
    r = read_ply(f)
    assert np.array_equal(r["points"], p) and r["normals"] is None and r["colors"] is None
    write_ply(f, np.zeros((0, 3), np.float32), binary=binary)
    assert len(read_ply(f)["points"]) == 0


def test_cpp_header_interoperates(tmp_path, hip_lib, orc):
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    p, nr, c = _cloud(777, 3)
    for binary_in in (True, False):
        for binary_out in (1, 0):
            a, b = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
            write_ply(a, p, nr, c, binary=binary_in)
            out = subprocess.run([BIN, "copy", a, b, str(binary_out)], capture_output=True, text=True, timeout=60)
            assert out.returncode == 0 and "777 points normals=1 colors=1" in out.stdout, out.stdout + out.stderr
            r = read_ply(b)
            assert np.array_equal(r["points"], p) and np.array_equal(r["normals"], nr)
            assert np.abs(r["colors"] - c).max() <= 1.0 / 255.0 + 1e-6
    # a file written by the C++ header alone, read back by Python
    w = str(tmp_path / "w.ply")
    assert subprocess.run([BIN, "write", w, "1"], timeout=60).returncode == 0
    r = read_ply(w)
    assert r["points"].shape == (1000, 3) and r["normals"] is not None and r["colors"] is not None
    assert np.all(r["normals"][:, 2] == 1.0)


def test_reads_the_references_test_cloud(tmp_path):
    """examples/test_clouds/frame_1.ply (binary little endian, xyz + normals + uchar rgb), rebuilt byte for byte from the committed
    fixtures (its header and colours: ref_nanoflann_golden.npz, its points and normals: frames_full.npz) and checked by its SHA-256"""
    import hashlib

    gold = os.path.join(ROOT, "tests", "golden")
    g, fr = np.load(os.path.join(gold, "ref_nanoflann_golden.npz")), np.load(os.path.join(gold, "frames_full.npz"))
    body = np.zeros(len(g["frame1_colors"]), np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    body["p"], body["n"], body["c"] = fr["p1"], fr["n1"], g["frame1_colors"]
    raw = g["frame1_ply_header"].tobytes() + body.tobytes()
    assert hashlib.sha256(raw).digest() == g["frame1_sha256"].tobytes()
    f = str(tmp_path / "frame_1.ply")
    open(f, "wb").write(raw)
    r = read_ply(f)
    assert r["points"].shape == (120111, 3) and r["normals"].shape == (120111, 3) and r["colors"].shape == (120111, 3)
    ok = np.isfinite(r["normals"]).all(axis=1)
    assert np.abs(np.linalg.norm(r["normals"][ok], axis=1) - 1).max() < 1e-3


def test_malformed_element_count_is_rejected(tmp_path, hip_lib, orc):
    """An element count the file cannot hold (crafted so that 3 * count wraps, or merely huge) is a malformed file:
    both readers refuse it before allocating or writing anything."""
    subprocess.check_call(["bash", os.path.join(ROOT, "tests", "cpp", "build.sh")])
    p, _, _ = _cloud(10)
    for count in (6148914691236517206, 1 << 40):       # ~2^64 / 3 (the product wraps in size_t), and a huge valid one
        for binary in (True, False):
            f = str(tmp_path / "bad.ply")
            write_ply(f, p, binary=binary)
            raw = open(f, "rb").read().replace(b"element vertex 10\n", b"element vertex %d\n" % count)
            open(f, "wb").write(raw)
            with pytest.raises(ValueError):
                read_ply(f)
            out = subprocess.run([BIN, "copy", f, str(tmp_path / "o.ply"), "1"], capture_output=True, text=True, timeout=60)
            assert out.returncode == 1 and "exceeds the file size" in out.stdout, out.stdout + out.stderr
