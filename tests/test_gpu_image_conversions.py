"""GPU: the image conversions (cilhip_depth_image_to_points3f, cilhip_points_to_depth_image3f, cilhip_points_to_index_map3f and their
Python / C++ mirrors) against the numpy restatement of tests/_projective_refs.py, bit for bit (NaN matching NaN).  The restatement is
pinned against a literal transcription of the reference's loops by tests/test_projective_refs_cpu.py."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _projective_refs as R
from test_projective_refs_cpu import GOLDEN, same

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
E_SMALL = R.small_E()
SHAPES = [(1, 1), (2, 5), (5, 2), (3, 3), (67, 5), (130, 3), (64, 64), (27, 19)]      # 27 x 19 = 513: two full blocks of 256 pixels and one pixel


@pytest.fixture(scope="module")
def ic():
    from cilantro_amd import image_conversions

    return image_conversions


@pytest.fixture(scope="module")
def frames():
    d = np.load(GOLDEN)
    return d["p1"], d["p2"]


@pytest.fixture(scope="module")
def p1_depth(frames):
    """p1 rendered by the restatement with the fusion camera, millimetres (computed once, never changed)"""
    depth, _ = R.points_to_depth_image(frames[0], R.FUSION_K, R.Conv(R.U16, 1000.0), 640, 480)
    depth.setflags(write=False)
    return depth.reshape(480, 640)


def mirror_conv(ic, c):
    return ic.TruncatedDepthValueConverter(float(c.scale), float(c.max_depth)) if c.truncated else ic.DepthValueConverter(float(c.scale))


def cuda(a, as_int16=False):
    import torch

    a = np.array(a, order="C")      # (a copy: fixtures are read-only)
    return torch.from_numpy(a.view(np.int16) if as_int16 else a).cuda()


def host(x):
    return None if x is None else (x.cpu().numpy() if hasattr(x, "cpu") else x)


def camera(w, h):
    return np.array([[0.8 * max(w, h) + 0.25, 0, (w - 1) / 2], [0, 0.75 * max(w, h) + 0.5, (h - 1) / 2], [0, 0, 1]], F)


def depth_patterns(w, h):
    """name -> (depth (h, w), converter)"""
    rng = np.random.default_rng(w * 1000 + h)
    valid = rng.integers(500, 2500, size=(h, w)).astype(np.uint16)
    mm = R.Conv(R.U16, 1000.0)
    out = {"zero": (np.zeros((h, w), np.uint16), mm), "valid": (valid, mm)}
    checker = valid.copy()
    checker[(np.add.outer(np.arange(h), np.arange(w)) % 2) == 1] = 0
    out["checker"] = (checker, mm)
    single = np.zeros((h, w), np.uint16)
    single[h // 2, w // 2] = 1234
    out["single"] = (single, mm)
    halves = np.where(np.arange(w)[None, :] * 2 < w, np.uint16(900), np.uint16(1900)) + (valid % 64)
    out["truncated"] = (halves.astype(np.uint16), R.Conv(R.U16, 1000.0, True, 1.5))
    out["max"] = (np.full((h, w), 65535, np.uint16), R.Conv(R.U16, 5000.0))
    raw = (valid.astype(F) / F(1000)).astype(F)
    flat = raw.reshape(-1)
    specials = np.array([np.nan, np.inf, -np.inf, -1.5, -0.0], F)
    flat[::3] = specials[np.arange(flat[::3].size) % 5]
    out["f32"] = (raw, R.Conv(R.F32, 1.0))
    out["f32-truncated"] = (raw, R.Conv(R.F32, 0.5, True, 3.0))
    return out


def check_to_points(ic, depth, conv, K, rgb, E, keep_invalid, want_normals, device_mem):
    h, w = depth.shape
    want = R.depth_to_points(depth, w, h, K, conv, rgb=rgb, E=E, keep_invalid=keep_invalid, want_normals=want_normals)
    d_in, c_in = depth, rgb
    if device_mem:
        d_in, c_in = cuda(depth, as_int16=depth.dtype == np.uint16), None if rgb is None else cuda(rgb)
    got = ic.depth_image_to_points(d_in, mirror_conv(ic, conv), K, E, c_in, keep_invalid, want_normals)
    if device_mem:
        assert all(g is None or g.is_cuda for g in got)
    for g, r, name in zip(got, want, ("points", "normals", "colors")):
        assert same(host(g), r), (name, depth.shape, keep_invalid, want_normals, E is not None, device_mem)
    return want


@pytest.mark.parametrize("w,h", SHAPES, ids=lambda v: str(v))
def test_depth_to_points_every_pattern_and_variant(ic, w, h):
    K = camera(w, h)
    rgb = np.random.default_rng(9).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    rows = {}
    for name, (depth, conv) in depth_patterns(w, h).items():
        for k, (keep_invalid, want_normals, with_rgb, with_e) in enumerate(itertools.product((False, True), repeat=4)):
            device_mem = (k % 3 == 0) if (w, h) != (64, 64) else (k % 2 == 1)
            got = check_to_points(ic, depth, conv, K, rgb if with_rgb else None, E_SMALL if with_e else None, keep_invalid, want_normals, device_mem)
            rows[(name, keep_invalid, want_normals)] = got[0].shape[0]
    assert rows[("zero", False, False)] == 0 and rows[("valid", False, False)] == w * h and rows[("single", False, False)] == 1
    assert rows[("valid", True, True)] == w * h
    assert rows[("valid", False, True)] == (max(w - 2, 0) * max(h - 2, 0) if min(w, h) >= 3 else 0)
    assert rows[("truncated", False, False)] == ((w + 1) // 2) * h
    assert rows[("single", False, True)] == 0


def test_depth_to_points_full_frame(ic, p1_depth):
    conv = R.Conv(R.U16, 1000.0)
    rgb = np.random.default_rng(2).integers(0, 256, size=(480, 640, 3), dtype=np.uint8)
    want = check_to_points(ic, p1_depth, conv, R.FUSION_K, rgb, None, False, True, True)
    assert want[0].shape[0] == 113870
    assert check_to_points(ic, p1_depth, conv, R.FUSION_K, None, E_SMALL, False, False, False)[0].shape[0] == 118703
    # two runs: the same bits
    a = ic.depth_image_to_points(p1_depth, mirror_conv(ic, conv), R.FUSION_K, E_SMALL, rgb, False, True)
    b = ic.depth_image_to_points(p1_depth, mirror_conv(ic, conv), R.FUSION_K, E_SMALL, rgb, False, True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_capacity_protocol(hip_lib):
    from cilantro_amd import capi

    w, h = 67, 5
    depth, conv = depth_patterns(w, h)["checker"]
    want = R.depth_to_points(depth, w, h, camera(w, h), conv)[0]
    c = capi.DepthConverter(capi.DEPTH_U16, 1000.0, 0, 0.0)
    K = np.ascontiguousarray(camera(w, h).T)
    n_out = C.c_size_t(0)
    call = lambda out, cap: hip_lib.cilhip_depth_image_to_points3f(0, depth.ctypes.data, None, w, h, capi.MEM_HOST, C.byref(c), K.ctypes.data, None, 0, 0,      # noqa: E731
                                                                   None if out is None else out.ctypes.data, None, None, cap, C.byref(n_out))
    assert call(None, 0) == capi.OK and n_out.value == want.shape[0] > 0      # the counting call
    small = np.full((want.shape[0], 3), 7, F)
    n_out.value = 0
    assert call(small, want.shape[0] - 1) == capi.ERR_INVALID and n_out.value == want.shape[0] and (small == 7).all()
    assert b"capacity" in hip_lib.cilhip_last_error(None)
    assert call(small, want.shape[0]) == capi.OK and same(small, want)


# ---- points -> image -------------------------------------------------------------------------------------------------------------
def check_to_image(ic, p, K, w, h, E=None, conv=None, colours=None, device_mem=False):
    """the index map and (with a converter) the depth / rgb image of one cloud against the restatement"""
    pin, cin = (cuda(p), None if colours is None else cuda(colours)) if device_mem else (p, colours)
    got = host(ic.points_to_index_map(pin, K, w, h, E)).view(np.uint32) if device_mem else ic.points_to_index_map(pin, K, w, h, E)
    want = R.points_to_index_map(p, K, w, h, E)
    assert np.array_equal(got.reshape(-1), want)
    if conv is None:
        return want
    depth, rgb = ic.points_to_depth_image(pin, K, mirror_conv(ic, conv), w, h, E, cin, conv.dtype)
    wd, wc = R.points_to_depth_image(p, K, conv, w, h, E, colours)
    depth = host(depth)
    assert same(depth.view(conv.dtype).reshape(-1), wd)
    assert (rgb is None and wc is None) or np.array_equal(host(rgb).reshape(-1, 3), wc)
    return want


def test_one_point(ic):
    K = camera(4, 3)
    p = np.array([[0.0, 0.0, 1.25]], F)
    im = check_to_image(ic, p, K, 4, 3, conv=R.Conv(R.U16, 1000.0), colours=np.array([[0.2, 0.5, 1.0]], F))
    assert (im != R.EMPTY).sum() == 1


@pytest.mark.parametrize("device_mem", [False, True])
def test_contention_and_ties_in_one_pixel(ic, device_mem):
    """4096 points into ONE pixel of a 4 x 3 image, z drawn from 8 values"""
    rng = np.random.default_rng(11)
    z = rng.choice(np.linspace(0.75, 1.625, 8).astype(F), 4096).astype(F)
    K = camera(4, 3)
    p = np.stack([z * F(0.01), z * F(-0.01), z], axis=1).astype(F)      # the ray of pixel (2, 1), a little off centre
    col = rng.random((4096, 3)).astype(F)
    im = check_to_image(ic, p, K, 4, 3, conv=R.Conv(R.U16, 4.0), colours=col, device_mem=device_mem)      # (scale 4: pairs of z share a raw value)
    assert (im != R.EMPTY).sum() == 1 and im[im != R.EMPTY][0] == np.flatnonzero(z == z.min())[0]
    check_to_image(ic, p, K, 4, 3, E=E_SMALL, conv=R.Conv(R.F32, 2.0), colours=col, device_mem=device_mem)


def test_behind_the_camera_and_rounding_boundaries(ic):
    K1 = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    w = 4
    us = np.array([-0.4, -0.5, 0.5, 1.5, 2.5, w - 0.5, w - 0.75, np.nextafter(F(0.5), F(0))], F)
    p = np.stack([us, np.zeros_like(us), np.ones_like(us)], axis=1)
    im = check_to_image(ic, p, K1, w, 1, conv=R.Conv(R.U16, 100.0))
    assert im.tolist() == [0, 2, 3, 4]      # -0.4 -> pixel 0 (before 0.49999997, by index); 2.5 -> 3 beats w - 0.75 by index
    behind = np.array([[0.1, 0.1, -1.0], [0.0, 0.0, 0.0], [0.0, 0.0, -0.0], [np.nan, 0, 1], [0, 0, np.nan], [0, 0, np.inf], [1e30, 0, 1e-30]], F)
    im = check_to_image(ic, behind, camera(5, 4), 5, 4, conv=R.Conv(R.F32, 1.0))
    assert (im == R.EMPTY).all()
    both = np.concatenate([behind, np.array([[0, 0, 2.0]], F)])
    assert (check_to_image(ic, both, camera(5, 4), 5, 4, E=E_SMALL, conv=R.Conv(R.F32, 1.0)) != R.EMPTY).sum() == 1


def test_overflow_truncation_and_colour_saturation(ic):
    rng = np.random.default_rng(4)
    p = np.stack([rng.uniform(-0.4, 0.4, 500), rng.uniform(-0.3, 0.3, 500), rng.uniform(0.5, 3.0, 500)], axis=1).astype(F)
    col = rng.uniform(-0.5, 1.5, (500, 3)).astype(F)
    col[::7] = np.array([np.nan, np.inf, -np.inf], F)
    K = camera(9, 7)
    # scale 40000: every z >= 1.6384 overflows u16 and is skipped
    for conv in (R.Conv(R.U16, 40000.0), R.Conv(R.U16, 1000.0, True, 1.75), R.Conv(R.F32, 1000.0, True, 2.0), R.Conv(R.U16, 0.25)):
        check_to_image(ic, p, K, 9, 7, conv=conv, colours=col)
    d, _ = R.points_to_depth_image(p, K, R.Conv(R.U16, 40000.0), 9, 7)
    assert 0 < np.count_nonzero(d) and (R.points_to_depth_image(p, K, R.Conv(R.U16, 0.25), 9, 7)[0] == 0).all()


@pytest.mark.parametrize("case", ["default-K", "fusion-K", "fusion-K-E"])
def test_frames_full(ic, frames, case):
    p1 = frames[0]
    K = R.DEFAULT_K if case == "default-K" else R.FUSION_K
    E = E_SMALL if case.endswith("-E") else None
    col = np.random.default_rng(1).random(p1.shape).astype(F)
    im = check_to_image(ic, p1, K, 640, 480, E=E, conv=R.Conv(R.U16, 1000.0), colours=col, device_mem=(case == "fusion-K"))
    if case == "fusion-K":
        assert (im != R.EMPTY).sum() == 118703
    a, b = ic.points_to_index_map(p1, K, 640, 480, E), ic.points_to_index_map(p1, K, 640, 480, E)
    assert a.tobytes() == b.tobytes()


def test_round_trip_on_a_ray_cast_scene(ic):
    depth, K = R.raycast_scene()
    conv = ic.DepthValueConverter(1000.0)
    pts = ic.depthImageToPoints(depth, conv, K)
    assert pts.shape[0] == 67 * 45
    assert np.array_equal(ic.pointsToDepthImage(pts, K, conv, 67, 45), depth)
    rgb = np.random.default_rng(3).integers(0, 256, size=(45, 67, 3), dtype=np.uint8)
    p, n, c = ic.RGBDImagesToPointsNormalsColors(rgb, depth, conv, K, keep_invalid=True)
    back_rgb, back = ic.pointsColorsToRGBDImages(p, c, K, conv, 67, 45)
    assert np.array_equal(back, depth)
    # 255 * ((1 / 255) * b) truncates to b or b - 1
    assert (np.abs(back_rgb.astype(int) - rgb.astype(int)) <= 1).all()
    assert np.array_equal(ic.pointsToIndexMap(p, K, 67, 45).reshape(-1), np.arange(67 * 45, dtype=np.uint32))


def test_stateless_calls_leave_no_allocation(ic, hip_lib, frames):
    live = (C.c_ulonglong * 2)()
    hip_lib.cilhip_debug_live_allocations(live)
    before = tuple(live)
    depth, K = R.raycast_scene()
    conv = ic.DepthValueConverter(1000.0)
    p, n = ic.depthImageToPointsNormals(depth, conv, K, extrinsics=E_SMALL)
    ic.pointsToDepthImage(p, K, conv, 67, 45, extrinsics=E_SMALL)
    ic.pointsToIndexMap(cuda(frames[0]), R.FUSION_K, 640, 480)
    hip_lib.cilhip_debug_live_allocations(live)
    assert tuple(live) == before


def test_cpp_mirror_gives_the_python_mirror_results(ic, tmp_path):
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_image_conversions.cpp"), "test_image_conversions")
    depth, K = R.raycast_scene()
    depth = depth.copy()
    depth[::4, ::5] = 0      # holes
    rgb = np.random.default_rng(8).integers(0, 256, size=(45, 67, 3), dtype=np.uint8)
    pre = str(tmp_path / "out")
    files = {"depth.u16": depth, "rgb.u8": rgb, "K.f32": np.ascontiguousarray(K.T), "E.f32": np.ascontiguousarray(E_SMALL.T)}
    for name, a in files.items():
        a.tofile(str(tmp_path / name))
    r = subprocess.run([exe, "run"] + [str(tmp_path / n) for n in ("depth.u16", "rgb.u8")] + ["67", "45", str(tmp_path / "K.f32"), str(tmp_path / "E.f32"), "1000", pre],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
    conv = ic.DepthValueConverter(1000.0)
    p, n, c = ic.RGBDImagesToPointsNormalsColors(rgb, depth, conv, K)
    f32 = lambda v: np.fromfile(f"{pre}.{v}.f32", F).reshape(-1, 3)      # noqa: E731
    assert 0 < p.shape[0] < 67 * 45 and same(f32("points"), p) and same(f32("normals"), n) and same(f32("colors"), c)
    wp, wn = ic.depthImageToPointsNormals(depth, conv, K, extrinsics=E_SMALL, keep_invalid=True)
    assert same(f32("world"), wp) and same(f32("world_normals"), wn)
    back_rgb, back = ic.pointsColorsToRGBDImages(p, c, K, conv, 67, 45)
    assert np.array_equal(np.fromfile(pre + ".depth.u16", np.uint16), back.reshape(-1)) and np.array_equal(np.fromfile(pre + ".rgb.u8", np.uint8), back_rgb.reshape(-1))
    index = ic.pointsToIndexMap(wp, K, 67, 45, extrinsics=E_SMALL).reshape(-1).astype(np.uint64)
    index[index == R.EMPTY] = np.iinfo(np.uint64).max      # the mirrors present size_t with SIZE_MAX
    assert np.array_equal(np.fromfile(pre + ".index.u64", np.uint64), index)
