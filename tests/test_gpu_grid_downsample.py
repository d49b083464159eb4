"""GPU: the voxel-grid downsampler (cilhip_grid_downsample3f and its Python / C++ mirrors) against the numpy restatement of the
reference (tests/_grid_refs.py, pinned on the CPU by tests/test_grid_downsample_cpu.py).  The contract is exact, so every
comparison is np.array_equal on uint32 views -- points, normals, colours, counts and the number of rows; no tolerance."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from _grid_refs import grid_downsample_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
WAVE_MIN = 64      # csrc/grid_downsample.hip GD_WAVE_MIN: bins with more members are folded by a whole wave, the others by one lane


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


@pytest.fixture(scope="module")
def L():
    from cilantro_amd import capi

    return capi.load()


@pytest.fixture(scope="module")
def frame():
    f = np.load(os.path.join(HERE, "golden", "frames_full.npz"))
    p, n = f["p1"], f["n1"]
    c = np.random.default_rng(11).random(p.shape, dtype=np.float32)
    return p, n, c


def flip_signs(n):
    sign = np.where(np.random.default_rng(7).random(n.shape[0]) < 0.5, np.float32(-1.0), np.float32(1.0))[:, None]
    return (n * sign).astype(np.float32)


def run(L, pts, nrm, col, bin_size, min_pts=1, lex=True, capacity=None, outputs=True, fill=None):
    """the C entry with host pointers -> (rc, rows, [points, normals, colours, counts] cut to the rows, the full buffers)"""
    pts = np.ascontiguousarray(pts, np.float32)
    n = pts.shape[0]
    cap = n if capacity is None else capacity
    alloc = lambda cols, dt: (np.full((max(cap, 1), cols) if cols else (max(cap, 1),), 0 if fill is None else fill, dt))      # noqa: E731
    bufs = [alloc(3, np.float32), alloc(3, np.float32) if nrm is not None else None, alloc(3, np.float32) if col is not None else None, alloc(0, np.uint32)]
    if not outputs:
        bufs = [None, None, None, None]
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data      # noqa: E731
    keep = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (nrm, col)]
    rows = C.c_size_t(0)
    rc = L.cilhip_grid_downsample3f(0, pts.ctypes.data, ptr(keep[0]), ptr(keep[1]), n, 0, C.c_float(bin_size), min_pts, 1 if lex else 0,
                                    *[None if b is None else b.ctypes.data for b in bufs], cap, C.byref(rows))
    m = rows.value
    cut = [None if b is None else b[:m] for b in bufs] if rc == 0 else None
    return rc, m, cut, bufs


def check(L, pts, nrm, col, bin_size, min_pts=1, lex=True, ref=None):
    """one call against the restatement, bit for bit -> the counts"""
    if ref is None:
        ref = grid_downsample_ref(pts, nrm, col, bin_size, min_pts, lex)
    rc, m, out, _ = run(L, pts, nrm, col, bin_size, min_pts, lex)
    assert rc == 0, L.cilhip_last_error(None)
    assert m == ref[0].shape[0]
    assert same_bits(out[0], ref[0]), "points"
    if nrm is not None:
        assert same_bits(out[1], ref[1]), "normals"
    if col is not None:
        assert same_bits(out[2], ref[2]), "colours"
    assert np.array_equal(out[3], ref[3]), "counts"
    return out[3]


# ---- the reference's sensor frame ----------------------------------------------------------------------------------
@pytest.mark.parametrize("lex", [True, False])
@pytest.mark.parametrize("bin_size,bins,largest", [(0.005, 15531, 30), (0.01, 4409, 105), (0.05, 251, 1767)])
def test_sensor_frame(L, frame, bin_size, bins, largest, lex):
    p, n, c = frame
    for min_pts in (1, 3):
        ref = grid_downsample_ref(p, n, c, bin_size, min_pts, lex)
        if min_pts == 1:
            assert ref[0].shape[0] == bins and int(ref[3].max()) == largest
        for use_n, use_c in ((False, False), (True, False), (False, True), (True, True)):
            cnt = check(L, p, n if use_n else None, c if use_c else None, bin_size, min_pts, lex, ref=ref)
        if largest > WAVE_MIN:      # both fold forms are met: bins on either side of the switch-over
            assert (cnt > WAVE_MIN).any() and (cnt <= WAVE_MIN).any()
        else:
            assert (cnt <= WAVE_MIN).all()
    # the normal rule's subtracting branch: random signs on the input normals
    check(L, p, flip_signs(n), c, bin_size, 1, lex)


def test_fold_forms_at_the_chunk_edges(L):
    """bins of 1 .. 1000 members around the lane / wave switch-over and the wave form's 64-member chunks, members interleaved in input order"""
    rng = np.random.default_rng(5)
    sizes = [1, 2, 3, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000]
    cell = np.repeat(np.arange(len(sizes)), sizes)
    p = np.zeros((cell.size, 3), np.float32)
    p[:, 0] = (cell - 7 + rng.random(cell.size) * 0.98 + 0.01) * 0.1
    p[:, 1:] = rng.random((cell.size, 2)) * 0.09 - 0.3
    nrm = rng.normal(size=p.shape).astype(np.float32) * np.float32(0.3) + np.array([0, 0, 1], np.float32)
    nrm = flip_signs((nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32))
    col = rng.random(p.shape, dtype=np.float32)
    sh = rng.permutation(cell.size)
    p, nrm, col = p[sh], nrm[sh], col[sh]
    for lex in (True, False):
        for use_n, use_c in ((False, False), (True, False), (False, True), (True, True)):
            cnt = check(L, p, nrm if use_n else None, col if use_c else None, 0.1, 1, lex)
            assert sorted(cnt.tolist()) == sorted(sizes)
        check(L, p, nrm, col, 0.1, 64, lex)
        check(L, p, nrm, col, 0.1, 65, lex)


# ---- memory spaces, repeatability, the capacity protocol ------------------------------------------------------------------
def test_host_device_repeat_and_capacity(L, frame):
    import torch
    from cilantro_amd import capi
    from cilantro_amd import grid_downsampler as gd

    p, n, c = frame
    ref = grid_downsample_ref(p, n, c, 0.01, 1, True)
    bins = ref[0].shape[0]
    a = gd.grid_downsample(p, 0.01, normals=n, colors=c)
    b = gd.grid_downsample(p, 0.01, normals=n, colors=c)
    tp, tn, tc = (torch.from_numpy(x).cuda() for x in (p, n, c))
    d = gd.grid_downsample(tp, 0.01, normals=tn, colors=tc)
    assert all(isinstance(a[k], np.ndarray) for k in a) and all(d[k].is_cuda for k in d)
    for k, r in (("points", ref[0]), ("normals", ref[1]), ("colors", ref[2])):
        assert same_bits(a[k], r) and same_bits(b[k], r) and same_bits(d[k].cpu().numpy(), r), k
    # torch tensors on the host are host arrays
    h = gd.grid_downsample(torch.from_numpy(p), 0.01)
    assert same_bits(np.asarray(h["points"]), ref[0]) and h["normals"] is None and h["colors"] is None
    # a downsampler object: one device pass, every getter and every min_points_in_bin from it; host and device alike
    r3 = grid_downsample_ref(p, n, c, 0.01, 3, False)
    r1 = grid_downsample_ref(p, n, c, 0.01, 1, False)
    for dev in (False, True):
        args = (tp, tn, tc) if dev else (p, n, c)
        get = (lambda x: x.cpu().numpy()) if dev else (lambda x: x)
        ds = gd.PointsNormalsColorsGridDownsampler3f(*args, 0.01, parallel=False)
        assert ds.getNumberOfOccupiedBins() == r1[0].shape[0]
        assert np.array_equal(u32(get(ds.getBinPointCounts())), r1[3])
        for mp, r in ((1, r1), (3, r3)):
            P, N, Cc = ds.getDownsampledPointsNormalsColors(mp)
            assert same_bits(get(P), r[0]) and same_bits(get(N), r[1]) and same_bits(get(Cc), r[2])
            assert same_bits(get(ds.getDownsampledPoints(mp)), r[0]) and same_bits(get(ds.getDownsampledNormals(mp)), r[1]) and same_bits(get(ds.getDownsampledColors(mp)), r[2])
        dn = gd.PointsNormalsGridDownsampler3f(args[0], args[1], 0.01, parallel=False)
        P, N = dn.getDownsampledPointsNormals(3)
        assert same_bits(get(P), r3[0]) and same_bits(get(N), r3[1])
        dc = gd.PointsColorsGridDownsampler3f(args[0], args[2], 0.01, parallel=False)
        P, Cc = dc.getDownsampledPointsColors(3)
        assert same_bits(get(P), r3[0]) and same_bits(get(Cc), r3[2])
        assert same_bits(get(gd.PointsGridDownsampler3f(args[0], 0.01, parallel=False).getDownsampledPoints(3)), r3[0])
    # the counting call: every output null, capacity 0
    rc, m, _, _ = run(L, p, n, c, 0.01, outputs=False, capacity=0)
    assert rc == capi.OK and m == bins
    # capacity too small: refused, the count still reported, nothing written
    rc, m, _, bufs = run(L, p, n, c, 0.01, capacity=bins - 1, fill=7)
    assert rc == capi.ERR_INVALID and m == bins and b"capacity" in L.cilhip_last_error(None)
    assert all((x == 7).all() for x in bufs)
    # exactly enough, and capacity == n
    for cap in (bins, p.shape[0]):
        rc, m, out, bufs = run(L, p, n, c, 0.01, capacity=cap, fill=7)
        assert rc == capi.OK and m == bins and same_bits(out[0], ref[0]) and same_bits(out[1], ref[1]) and same_bits(out[2], ref[2]) and np.array_equal(out[3], ref[3])
        assert all((x[bins:] == 7).all() for x in bufs)      # nothing beyond the rows


# ---- past one grid trip, off the origin ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """4M points in [-1, 1]^2 x [-0.05, 0.05]: twice what one trip of the kernels' grids covers"""
    rng = np.random.default_rng(1)
    return (rng.random((4_000_000, 3), dtype=np.float32) * np.array([2, 2, 0.1], np.float32) - np.array([1, 1, 0.05], np.float32)).astype(np.float32)


def test_four_million_points(L, big):
    p = big
    rng = np.random.default_rng(2)
    nrm = rng.normal(size=p.shape).astype(np.float32)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    col = rng.random(p.shape, dtype=np.float32)
    ref = grid_downsample_ref(p, nrm, col, 0.01, 1, True)
    assert ref[0].shape[0] == 399979 and int(ref[3].max()) == 29
    cnt = check(L, p, nrm, col, 0.01, 1, True, ref=ref)
    assert (cnt <= WAVE_MIN).all()      # the lane form alone here; the wave form: test_sensor_frame, test_fold_forms_at_the_chunk_edges, test_extremes
    check(L, p, None, None, 0.01, 4, False)


@pytest.mark.parametrize("shift", [(1000.0, -500.0, 250.0), (0.0049, -0.0051, 0.0452)])
def test_four_million_points_moved(L, big, shift):
    """far from the origin (cells ~ 10^5, all of one sign per axis), and moved so that cell 0's boundary runs through the data on every axis"""
    p = (big + np.array(shift, np.float32)).astype(np.float32)
    col = np.random.default_rng(3).random(p.shape, dtype=np.float32)
    st = {}
    ref = grid_downsample_ref(p, None, col, 0.01, 1, True, stats=st)
    if abs(shift[0]) < 1.0:
        assert (st["cells"].min(axis=0) < 0).all() and (st["cells"].max(axis=0) >= 0).all()
    else:
        assert np.abs(st["cells"]).min() > 10000
    check(L, p, None, col, 0.01, 1, True, ref=ref)
    check(L, p, None, col, 0.01, 2, False)


def test_points_exactly_on_cell_boundaries(L):
    for bin_size in (0.25, 0.01, 0.005):
        k = np.arange(-300, 301)
        g = np.stack(np.meshgrid(k[::7], k[::11], k[::13], indexing="ij"), axis=-1).reshape(-1, 3)
        p = (g.astype(np.float32) * np.float32(bin_size)).astype(np.float32)      # k * bin_size, rounded to f32 as a user would form it
        p = np.concatenate([p, p[::3]])[np.random.default_rng(4).permutation(p.shape[0] + p[::3].shape[0])]
        for lex in (True, False):
            check(L, p, None, p, bin_size, 1, lex)


# ---- extremes ----------------------------------------------------------------------------------------------------------
def test_extremes(L):
    rng = np.random.default_rng(6)
    # every point its own bin: the outputs are the inputs, bit for bit, reordered; normals renormalised
    k = rng.permutation(200_000)[:50_000]
    p = np.stack([(k % 100) - 50, (k // 100) % 100 - 50, k // 10000], axis=1).astype(np.float32) + rng.random((50_000, 3), dtype=np.float32) * np.float32(0.9)
    nrm = rng.normal(size=p.shape).astype(np.float32)
    col = rng.random(p.shape, dtype=np.float32)
    rc, m, out, _ = run(L, p, nrm, col, 1.0, 1, False)
    assert rc == 0 and m == 50_000 and same_bits(out[0], p) and same_bits(out[2], col) and (out[3] == 1).all()
    z = nrm[:, 0] * nrm[:, 0] + (nrm[:, 1] * nrm[:, 1] + nrm[:, 2] * nrm[:, 2])
    assert same_bits(out[1], nrm / np.sqrt(z)[:, None])
    cnt = check(L, p, nrm, col, 1.0, 1, True)
    assert (cnt == 1).all()
    # min_points_in_bin above every count: no rows
    rc, m, _, bufs = run(L, p, nrm, col, 1.0, 2, True, fill=7)
    assert rc == 0 and m == 0 and all((x == 7).all() for x in bufs)
    # a million points in one bin: the plain running sum
    q = (rng.random((1_000_000, 3), dtype=np.float32) * np.float32(0.999)).astype(np.float32)
    rc, m, out, _ = run(L, q, None, q[::-1], 1.0, 1, True)
    acc = np.add.accumulate(q, axis=0, dtype=np.float32)[-1]
    acc_c = np.add.accumulate(q[::-1], axis=0, dtype=np.float32)[-1]
    scale = np.float32(1.0) / np.float32(1_000_000)
    assert rc == 0 and m == 1 and out[3][0] == 1_000_000
    assert same_bits(out[0][0], scale * acc) and same_bits(out[2][0], scale * acc_c)
    # ... and with the normal rule over a long bin (every decision made one member at a time)
    w = 20_000
    nq = flip_signs((np.array([0, 0, 1], np.float32) + rng.normal(size=(w, 3)).astype(np.float32) * np.float32(0.2)).astype(np.float32))
    check(L, q[:w], nq, None, 1.0, 1, False)
    # exact duplicates
    d = np.repeat(rng.random((1000, 3), dtype=np.float32), 5, axis=0)[rng.permutation(5000)]
    cnt = check(L, d, d, d, 0.05, 1, True)
    assert cnt.sum() == 5000
    # a lone -0.0f stays -0.0f (a sum starts AS its first member, scale 1)
    s = np.array([[-0.0, 0.5, 0.5], [10.5, -0.0, 0.5], [20.5, 0.5, -0.0]], np.float32)
    rc, m, out, _ = run(L, s, None, s, 1.0, 1, False)
    assert rc == 0 and m == 3 and same_bits(out[0], s) and same_bits(out[2], s)
    assert np.signbit(out[0][0, 0]) and np.signbit(out[0][1, 1]) and np.signbit(out[0][2, 2])
    # one point
    check(L, s[:1], s[:1], s[:1], 0.3, 1, True)


# ---- non-finite input ---------------------------------------------------------------------------------------------------
def test_non_finite_points_have_no_bin(L, frame):
    p, n, c = frame
    rng = np.random.default_rng(8)
    q = p.copy()
    bad = rng.permutation(q.shape[0])[: q.shape[0] // 100]
    q[bad, rng.integers(0, 3, bad.size)] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), bad.size)
    q[0] = np.nan      # the first point too: first-appearance order starts at the first FINITE point
    ok = np.isfinite(q).all(axis=1)
    assert 0 < (~ok).sum() < q.shape[0] // 50
    for lex in (True, False):
        for bin_size in (0.005, 0.05):
            ref = grid_downsample_ref(q[ok], n[ok], c[ok], bin_size, 1, lex)
            cnt = check(L, q, n, c, bin_size, 1, lex, ref=ref)
            assert int(cnt.sum(dtype=np.int64)) == int(ok.sum())
    check(L, q, None, None, 0.01, 3, True, ref=grid_downsample_ref(q[ok], None, None, 0.01, 3, True))
    # nothing but non-finite points: no rows
    rc, m, _, _ = run(L, np.full((1000, 3), np.nan, np.float32), None, None, 0.01)
    assert rc == 0 and m == 0


def test_non_finite_normals_stay_in_their_bins(L, frame):
    p, n, c = frame
    rng = np.random.default_rng(9)
    nn = n.copy()
    bad = rng.permutation(n.shape[0])[: n.shape[0] // 100]
    nn[bad, rng.integers(0, 3, bad.size)] = np.nan
    for lex in (True, False):
        clean = grid_downsample_ref(p, n, c, 0.005, 1, lex)
        ref = grid_downsample_ref(p, nn, c, 0.005, 1, lex)
        rc, m, out, _ = run(L, p, nn, c, 0.005, 1, lex)
        assert rc == 0 and m == clean[0].shape[0]
        assert same_bits(out[0], clean[0]) and same_bits(out[2], clean[2]) and np.array_equal(out[3], clean[3])      # points, colours, counts, order: unaffected
        nan_g, nan_r = np.isnan(out[1]), np.isnan(ref[1])
        assert np.array_equal(nan_g, nan_r) and nan_r.any() and not nan_r.all()      # the same bins' normals are NaN (a NaN's payload is not part of the contract)
        rows = ~nan_r.any(axis=1)
        assert same_bits(out[1][rows], ref[1][rows]) and same_bits(out[1][rows], clean[1][rows])


# ---- refusal on the device ------------------------------------------------------------------------------------------------
def test_out_of_range_cell_is_refused_without_a_trace(L):
    import torch
    from cilantro_amd import capi
    from cilantro_amd import grid_downsampler as gd

    rng = np.random.default_rng(10)
    p = rng.random((1_000_000, 3), dtype=np.float32)
    good = p.copy()
    p[777_777, 1] = np.float32(-3.0 * (1 << 20) * 0.01)
    rc, m, _, bufs = run(L, p, p, p, 0.01, fill=7)
    assert rc == capi.ERR_UNSUPPORTED and b"2^20" in L.cilhip_last_error(None)
    assert all((x == 7).all() for x in bufs)
    # the edge of the accepted range itself is fine: cells -2^20 and 2^20 - 1
    e = np.array([[-(1 << 20) * 0.5, 0, 0], [((1 << 20) - 1) * 0.5, 0, 0], [0, 0, 0]], np.float32)
    st = {}
    check(L, e, None, None, 0.5, 1, True, ref=grid_downsample_ref(e, None, None, 0.5, 1, True, stats=st))
    assert st["cells"][:, 0].min() == -(1 << 20) and st["cells"][:, 0].max() == (1 << 20) - 1
    rc, m, _, _ = run(L, e + np.array([[-0.5, 0, 0], [0, 0, 0], [0, 0, 0]], np.float32), None, None, 0.5)
    assert rc == capi.ERR_UNSUPPORTED
    rc, m, _, _ = run(L, e + np.array([[0, 0, 0], [0.5, 0, 0], [0, 0, 0]], np.float32), None, None, 0.5)
    assert rc == capi.ERR_UNSUPPORTED
    # device tensors: the mirror raises, and the next valid call in the same process is right
    with pytest.raises(capi.CilhipError) as ei:
        gd.grid_downsample(torch.from_numpy(p).cuda(), 0.01)
    assert ei.value.code == capi.ERR_UNSUPPORTED
    check(L, good, good, None, 0.01, 1, True)


def test_wide_spread_takes_the_long_sort_keys(L):
    """cells spread over most of the accepted range on all three axes: the sort key no longer fits 32 bits; with the range's two ends on
    every axis and a non-finite point it uses all 64"""
    rng = np.random.default_rng(12)
    base = (rng.uniform(-5000, 5000, (50_000, 3))).astype(np.float32)
    p = np.repeat(base, 4, axis=0)[rng.permutation(200_000)]
    col = rng.random(p.shape, dtype=np.float32)
    st = {}
    ref = grid_downsample_ref(p, col, col, 0.01, 1, True, stats=st)
    assert (st["cells"].max(axis=0) - st["cells"].min(axis=0) > (1 << 19)).all()      # 20 bits per axis
    cnt = check(L, p, col, col, 0.01, 1, True, ref=ref)
    assert cnt.max() >= 4
    check(L, p, col, col, 0.01, 2, False)
    lo, hi = -(1 << 20) * 0.5, ((1 << 20) - 1) * 0.5
    q = rng.uniform(lo, hi, (100_000, 3)).astype(np.float32).clip(lo, hi)
    q[:3] = lo
    q[3:6] = hi
    q = np.concatenate([q, q[:50_000]])
    ok = np.ones(q.shape[0], bool)
    ok[[10, 1000, 149_999]] = False
    qq = q.copy()
    qq[~ok, 1] = np.nan
    for lex in (True, False):
        st = {}
        ref = grid_downsample_ref(q[ok], None, q[ok], 0.5, 1, lex, stats=st)
        assert (st["cells"].min(axis=0) == -(1 << 20)).all() and (st["cells"].max(axis=0) == (1 << 20) - 1).all()      # 21 bits per axis
        check(L, qq, None, qq, 0.5, 1, lex, ref=ref)


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------
def test_cpp_mirror_gives_the_python_mirror_arrays(L, frame, tmp_path):
    from cilantro_amd import grid_downsampler as gd
    from cilantro_amd import ply_io
    from test_grid_downsample_cpu import build_cpp_test

    exe = build_cpp_test()
    p, n, c = frame
    ply = str(tmp_path / "frame.ply")
    ply_io.write_ply(ply, p, n, c)
    cloud = ply_io.read_ply(ply)      # (colours went through uchar: both sides read the file)
    P, N, Cc = cloud["points"], cloud["normals"], cloud["colors"]
    assert same_bits(P, p) and same_bits(N, n) and Cc is not None
    for bin_size, min_pts, parallel in ((0.005, 1, 1), (0.01, 3, 0)):
        pre = str(tmp_path / f"out_{min_pts}")
        r = subprocess.run([exe, "run", ply, pre, repr(bin_size), str(min_pts), str(parallel)], capture_output=True, text=True)
        assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
        load = lambda v, a: np.fromfile(f"{pre}.{v}.{a}.f32", np.float32).reshape(-1, 3)      # noqa: E731
        py = gd.grid_downsample(P, bin_size, normals=N, colors=Cc, min_points_in_bin=min_pts, parallel=bool(parallel))
        assert py["points"].shape[0] > 100
        for v in ("pnc", "cloud", "cloud_copy"):
            assert same_bits(load(v, "p"), py["points"]) and same_bits(load(v, "n"), py["normals"]) and same_bits(load(v, "c"), py["colors"]), v
        assert same_bits(load("p", "p"), py["points"]) and same_bits(load("pn", "p"), py["points"]) and same_bits(load("pc", "p"), py["points"])
        assert same_bits(load("pn", "n"), py["normals"]) and same_bits(load("pc", "c"), py["colors"])
        ref = grid_downsample_ref(P, N, Cc, bin_size, min_pts, bool(parallel))
        assert same_bits(py["points"], ref[0]) and same_bits(py["normals"], ref[1]) and same_bits(py["colors"], ref[2])


# ---- end to end: the reference example's own flow ---------------------------------------------------------------------------
def test_downsample_then_icp_as_the_reference_example_does(frame):
    """examples/rigid_icp.cpp:25-65, :103-125: gridDownsample(0.005), src = dst + 0.01 * jitter, dst keeps x > -0.4, src moved by tf_ref,
    point-to-plane ICP with the example's parameters.  The bound is the one the two existing recipe tests use (jitter-limited)."""
    import torch
    from cilantro_amd import grid_downsampler as gd
    from cilantro_amd.icp import SimpleCombinedMetricRigidICP3f

    p, n, _ = frame
    ds = gd.grid_downsample(torch.from_numpy(p).cuda(), 0.005, normals=torch.from_numpy(n).cuda())
    dpts, dn = ds["points"].cpu().numpy(), ds["normals"].cpu().numpy()
    assert dpts.shape == (15531, 3)
    rng = np.random.default_rng(20250629)
    src = (dpts + np.float32(0.01) * rng.uniform(-1, 1, dpts.shape).astype(np.float32)).astype(np.float32)
    keep = dpts[:, 0] > -0.4
    dst, dst_n = dpts[keep], dn[keep]
    T_ref = np.load(os.path.join(HERE, "golden", "frame1_c1.npz"))["T_ref"]
    src = (src @ T_ref[:3, :3].T + T_ref[:3, 3]).astype(np.float32)
    icp = SimpleCombinedMetricRigidICP3f(dst, dst_n, src)
    icp.setMaxNumberOfOptimizationStepIterations(1).setPointToPointMetricWeight(0.0).setPointToPlaneMetricWeight(1.0)
    icp.correspondenceSearchEngine().setMaxDistance(0.1 * 0.1)
    icp.setConvergenceTolerance(1e-4).setMaxNumberOfIterations(30)
    Tg = icp.estimate().getTransform()
    dist = np.linalg.norm(Tg.astype(np.float64) - np.linalg.inv(T_ref.astype(np.float64)))
    print(f"downsample + ICP: {dpts.shape[0]} points, {icp.getNumberOfPerformedIterations()} iterations, |T - inv(T_ref)|_F = {dist:.3e}")
    assert icp.hasConverged() and dist < 5e-3, dist
