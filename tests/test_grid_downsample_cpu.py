"""CPU: the voxel-grid downsampler's interface and argument rules (no device needed), its C++ mirror's build, and the numpy
restatement (tests/_grid_refs.py) the GPU tests compare against -- checked against itself and against conditions on the real
sensor frame the comparisons rely on."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _grid_refs import explicit_loop_ref, grid_downsample_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")
NAME = "cilhip_grid_downsample3f"


def _has_gpu():
    import torch

    return torch.cuda.is_available()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def build_cpp_test():
    """tests/cpp/test_grid_downsample.cpp with the g++ line tests/cpp/build.sh uses for test_icp -> the binary's path"""
    cpp = os.path.join(HERE, "cpp")
    os.makedirs(os.path.join(cpp, "bin"), exist_ok=True)
    from oracle import oracle as orc

    orc.lib()      # (-loracle, as in that line)
    out = os.path.join(cpp, "bin", "test_grid_downsample")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), os.path.join(cpp, "test_grid_downsample.cpp"), "-o", out,
           "-L" + os.path.join(ROOT, "cilantro_amd", "lib"), "-lcilantro_hip", "-L" + os.path.join(ROOT, "oracle"), "-loracle",
           "-Wl,-rpath," + os.path.join(ROOT, "cilantro_amd", "lib"), "-Wl,-rpath," + os.path.join(ROOT, "oracle"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib",
           "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


# ---- the interface -------------------------------------------------------------------------------------------------
def test_symbol_is_declared_listed_and_exported(hip_lib):
    from cilantro_amd import capi

    txt = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\b%s\s*\(" % NAME, txt)
    assert NAME in capi.SYMBOLS
    assert hasattr(C.CDLL(capi.LIB_PATH), NAME)
    # the header cites the reference lines the entry restates
    hdr = open(HEADER).read()
    for needle in ("grid_downsampler.hpp:118-126", "grid_accumulator.hpp:79", "common_accumulators.hpp:45-46", "point_cloud.hpp:247-266"):
        assert needle in hdr, needle


def _call(L, pts, bin_size=0.01, mem=0, order=1, n=None, null_points=False, min_pts=1):
    pts = np.ascontiguousarray(pts, np.float32)
    n = pts.shape[0] if n is None else n
    out = np.full((max(n, 1), 3), 7.0, np.float32)
    rows = C.c_size_t(12345)
    rc = L.cilhip_grid_downsample3f(0, None if null_points else pts.ctypes.data, None, None, n, mem, C.c_float(bin_size), min_pts, order, out.ctypes.data, None, None, None,
                                    n, C.byref(rows))
    return rc, rows.value, out


def test_argument_rules_need_no_device(hip_lib):
    from cilantro_amd import capi

    pts = np.random.default_rng(0).random((100, 3), dtype=np.float32)
    # n == 0: fine, zero bins, wherever it runs
    rc, rows, _ = _call(hip_lib, np.zeros((0, 3), np.float32))
    assert rc == capi.OK and rows == 0
    rc, rows, _ = _call(hip_lib, pts, n=0, null_points=True)
    assert rc == capi.OK and rows == 0
    bad = [dict(bin_size=0.0), dict(bin_size=-0.01), dict(bin_size=float("nan")), dict(bin_size=float("inf")), dict(bin_size=float("-inf")), dict(mem=2), dict(mem=-1),
           dict(order=2), dict(order=-1), dict(null_points=True)]
    for kw in bad:
        rc, rows, out = _call(hip_lib, pts, **kw)
        assert rc == capi.ERR_INVALID, kw
        assert rows == 12345 and (out == 7.0).all(), kw      # nothing written
        assert b"grid_downsample" in hip_lib.cilhip_last_error(None), kw
    # every rule has its own text
    texts = set()
    for kw in (dict(bin_size=0.0), dict(mem=2), dict(order=2), dict(null_points=True)):
        _call(hip_lib, pts, **kw)
        texts.add(hip_lib.cilhip_last_error(None))
    assert len(texts) == 4
    if (1 << 32) < C.c_size_t(-1).value:
        rc, rows, out = _call(hip_lib, pts, n=1 << 32)
        assert rc == capi.ERR_INVALID and rows == 12345
    rows = C.c_size_t(0)
    assert hip_lib.cilhip_grid_downsample3f(0, pts.ctypes.data, None, None, 100, 0, C.c_float(0.01), 1, 1, None, None, None, None, 0, None) == capi.ERR_INVALID


def test_without_a_device_it_fails_loudly(hip_lib):
    from cilantro_amd import capi
    from cilantro_amd import grid_downsampler as gd

    if _has_gpu():
        pytest.skip("a GPU is present")
    pts = np.random.default_rng(0).random((100, 3), dtype=np.float32)
    rc, rows, out = _call(hip_lib, pts)
    assert rc == capi.ERR_NO_DEVICE and (out == 7.0).all()
    with pytest.raises(capi.CilhipError):
        gd.PointsGridDownsampler3f(pts, 0.01)
    with pytest.raises(capi.CilhipError):
        gd.PointsNormalsGridDownsampler3f(pts, pts, 0.01)
    with pytest.raises(capi.CilhipError):
        gd.PointsColorsGridDownsampler3f(pts, pts, 0.01, parallel=False)
    with pytest.raises(capi.CilhipError):
        gd.PointsNormalsColorsGridDownsampler3f(pts, pts, pts, 0.01)
    with pytest.raises(capi.CilhipError):
        gd.grid_downsample(pts, 0.01, normals=pts)
    # an empty cloud needs no device
    r = gd.grid_downsample(np.zeros((0, 3), np.float32), 0.01)
    assert r["points"].shape == (0, 3) and r["normals"] is None and r["colors"] is None


def test_python_mirror_refuses_bad_arguments_before_any_device(hip_lib):
    from cilantro_amd import capi
    from cilantro_amd import grid_downsampler as gd

    pts = np.zeros((10, 3), np.float32)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(capi.CilhipError) as e:
            gd.grid_downsample(pts, bad)
        assert e.value.code == capi.ERR_INVALID and "bin_size" in str(e.value)
    with pytest.raises(ValueError):
        gd.grid_downsample(pts, 0.01, normals=np.zeros((9, 3), np.float32))


def test_cpp_mirror_builds_and_throws_without_a_device(hip_lib):
    exe = build_cpp_test()
    if not _has_gpu():
        r = subprocess.run([exe, "--expect-no-device"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "no-device OK" in r.stdout
    # the project's own C++ build still goes through, test_ply still without the library
    r = subprocess.run(["bash", os.path.join(HERE, "cpp", "build.sh")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    deps = subprocess.run(["ldd", os.path.join(HERE, "cpp", "bin", "test_ply")], capture_output=True, text=True).stdout
    assert "cilantro_hip" not in deps and "amdhip64" not in deps
    src = open(os.path.join(ROOT, "examples", "rigid_icp.cpp")).read()
    assert "dst.gridDownsample(0.005f);" in src and "no voxel" not in src


# ---- the restatement against itself ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frame():
    f = np.load(os.path.join(HERE, "golden", "frames_full.npz"))
    p, n = f["p1"], f["n1"]
    assert p.shape == (120111, 3) and np.isfinite(p).all() and np.isfinite(n).all()
    return p, n


def flip_signs(n):
    sign = np.where(np.random.default_rng(7).random(n.shape[0]) < 0.5, np.float32(-1.0), np.float32(1.0))[:, None]
    return (n * sign).astype(np.float32)


def test_restatement_agrees_with_a_member_by_member_loop(frame):
    p, n = frame
    sel = slice(0, 6000)
    c = np.random.default_rng(3).random((6000, 3), dtype=np.float32)
    a = grid_downsample_ref(p[sel], flip_signs(n[sel]), c, 0.02, 1, lexicographic=False)
    b = explicit_loop_ref(p[sel], flip_signs(n[sel]), c, 0.02)
    for x, y in zip(a, b):
        assert np.array_equal(u32(x), u32(y))
    assert a[3].max() > 8


@pytest.mark.parametrize("bin_size,bins,largest", [(0.005, 15531, 30), (0.01, 4409, 105), (0.05, 251, 1767)])
def test_restatement_on_the_sensor_frame(frame, bin_size, bins, largest):
    p, n = frame
    N = p.shape[0]
    st_lex, st_first, st_flip = {}, {}, {}
    lex = grid_downsample_ref(p, n, None, bin_size, 1, True, stats=st_lex)
    fst = grid_downsample_ref(p, n, None, bin_size, 1, False, stats=st_first)
    assert lex[0].shape == (bins, 3) and int(lex[3].max()) == largest
    assert int(lex[3].sum(dtype=np.int64)) == N and int(fst[3].sum(dtype=np.int64)) == N
    # lexicographic cells strictly increasing, x most significant
    c = st_lex["cells"]
    d = np.diff(c, axis=0)
    lead = np.where(d[:, 0] != 0, d[:, 0], np.where(d[:, 1] != 0, d[:, 1], d[:, 2]))
    assert (lead > 0).all()
    # first appearance: ascending lowest member index, starting with point 0
    assert st_first["first"][0] == 0 and (np.diff(st_first["first"]) > 0).all()
    # the two orders are the same rows, bit for bit
    def rows(r):
        a = np.concatenate([u32(r[0]), u32(r[1]), r[3][:, None]], axis=1)
        return a[np.lexsort(a.T[::-1])]
    assert np.array_equal(rows(lex), rows(fst))
    # the cell is floor(p * inv), not floor(p / bin_size): at the two finer sizes the frame tells them apart
    inv = np.float32(1.0) / np.float32(bin_size)
    differ = int((np.floor(p * inv) != np.floor(p / np.float32(bin_size))).any(axis=1).sum())
    print(f"bin {bin_size}: floor(p * inv) != floor(p / bin) for {differ} points")
    assert differ > 0 or bin_size > 0.02
    # min_points_in_bin leaves rows out and keeps the order of the others
    k3 = grid_downsample_ref(p, n, None, bin_size, 3, True)
    keep = lex[3] >= 3
    assert 0 < keep.sum() < bins
    for x, y in zip((lex[0], lex[1], lex[3]), (k3[0], k3[1], k3[3])):
        assert np.array_equal(u32(x[keep]), u32(y))
    # random signs on the input normals change every output normal by at most its sign, exactly
    flp = grid_downsample_ref(p, flip_signs(n), None, bin_size, 1, True, stats=st_flip)
    assert np.array_equal(u32(flp[0]), u32(lex[0])) and np.array_equal(flp[3], lex[3])
    same = (u32(flp[1]) == u32(lex[1])).all(axis=1)
    neg = (u32(flp[1]) == u32(-lex[1])).all(axis=1)
    assert (same | neg).all() and same.any() and neg.any()
    # conditions on the inputs the bit-exact GPU comparisons rely on: no sign decision anywhere near zero (an FMA could flip one
    # only below ~1e-7), and with the random signs the subtracting branch is really taken
    for st in (st_lex, st_flip):
        assert st["decisions"] == N - bins
        assert st["min_abs_dot"] >= 0.05, st["min_abs_dot"]
    assert 3 * st_flip["subtractions"] > st_flip["decisions"], (st_flip["subtractions"], st_flip["decisions"])
    print(f"bin {bin_size}: min |dot| {st_lex['min_abs_dot']:.4g} / {st_flip['min_abs_dot']:.4g} (random signs), subtractions {st_lex['subtractions']} / "
          f"{st_flip['subtractions']} of {st_flip['decisions']}")
    assert 100 * st_lex["subtractions"] < st_lex["decisions"]      # (the sensor's own normals hardly ever disagree inside a bin)


def test_restatement_corners():
    # a lone -0.0f stays -0.0f; a sum starts as its first member
    p = np.array([[-0.0, 0.5, 0.5], [10.5, -0.0, 0.5]], np.float32)
    r = grid_downsample_ref(p, None, p, 1.0, 1, False)
    assert np.array_equal(u32(r[0]), u32(p)) and np.array_equal(u32(r[2]), u32(p))
    # points exactly on cell boundaries belong to the cell that starts there, negative ones included
    k = np.arange(-5, 6, dtype=np.float32)
    p = np.stack([k * np.float32(0.25), np.zeros_like(k), np.zeros_like(k)], axis=1)
    st = {}
    r = grid_downsample_ref(p, None, None, 0.25, 1, True, stats=st)
    assert np.array_equal(st["cells"][:, 0], np.arange(-5, 6)) and (r[3] == 1).all()
    # a zero normal sum stays as it is (normalized() of a zero vector)
    p = np.zeros((2, 3), np.float32) + np.float32(0.5)
    n = np.array([[0, 0, 1], [0, 0, -1]], np.float32)
    r = grid_downsample_ref(p, n, None, 1.0, 1, True)
    assert np.array_equal(r[1], np.array([[0, 0, 1]], np.float32))      # dot < 0: subtracted -> (0, 0, 2) -> normalised
    n = np.array([[0, 0, 0], [0, 0, 0]], np.float32)
    assert np.array_equal(grid_downsample_ref(p, n, None, 1.0, 1, True)[1], np.zeros((1, 3), np.float32))
