"""GPU: cilhip_kmeans_nd (rule S6) and its mirrors at every dimension, accumulator width, size edge, tie and
non-finite input, against the restatement tests/_spectral_refs.py::kmeans_nd.  Every comparison is exact -- labels, iteration counts and
centroids as bit patterns, a NaN matching a NaN: the f32 distance is pinned, the sums are f64 in a fixed order, the division is on the host.
The inputs and the restatement's runs come from tests/_kmeans_nd_refs.py (made once, shared, read-only);
tests/test_kmeans_nd_refs_cpu.py asserts of each input that it does what it was built to do.  Each test prints its figures before it
asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _kmeans_nd_refs as K
import _spectral_refs as R
from cilantro_amd import capi
from test_components_refs_cpu import build_cpp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
UNTOUCHED = 0xA5A5A5A5


def entry(x, start, max_iter, tol, labels=True, iterations=True):
    """cilhip_kmeans_nd on host arrays -> (centroids, labels or None, iterations or None)"""
    L = capi.load()
    n, D = x.shape
    cent = np.array(start, F32, order="C", copy=True)
    lab = np.full(n + 1, UNTOUCHED, np.uint32)
    it = C.c_size_t(UNTOUCHED)
    rc = L.cilhip_kmeans_nd(0, x.ctypes.data, n, D, capi.MEM_HOST, cent.ctypes.data, len(cent), int(max_iter), C.c_float(tol), lab.ctypes.data if labels else None,
                            C.byref(it) if iterations else None)
    assert rc == capi.OK, L.cilhip_last_error(None)
    assert lab[n] == UNTOUCHED and (labels or (lab == UNTOUCHED).all()) and (iterations or it.value == UNTOUCHED)
    return cent, (lab[:n].astype(np.int64) if labels else None), (int(it.value) if iterations else None)


def check(name):
    """one case through the C entry, bit for bit against the restatement -> (centroids, labels, iterations)"""
    x, s, max_iter, tol = K.case(name)
    want_c, want_l, want_it, _ = K.want(name)
    c, l, it = entry(x, s, max_iter, tol)
    nan = np.isnan(want_c)
    print(name, x.shape, "k", len(s), "iterations", it, want_it, "labels differing", int((l != want_l).sum()), "NaN pattern differs", int((np.isnan(c) != nan).sum()),
          "centroid words differing", int((c.view(np.uint32)[~nan] != want_c.view(np.uint32)[~nan]).sum()))
    assert it == want_it, name
    assert (l == want_l).all(), (name, np.flatnonzero(l != want_l)[:8].tolist())
    assert K.same_bits(c, want_c), (name, np.argwhere(c.view(np.uint32) != want_c.view(np.uint32))[:8].tolist())
    return c, l, it


# ---- 1: every dimension ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.DIMS)
def test_every_dimension(D):
    """1500 x D, k = 5: a start from the data and one whose last centroid is empty after the first pass, default tolerance and tol = 0"""
    for start in ("data", "far"):
        for tol in ("eps", "tol0"):
            check("dim-%d-%s-%s" % (D, start, tol))


# ---- 2: accumulator width ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,k", K.WIDTHS, ids=["%dx%d" % w for w in K.WIDTHS])
def test_accumulator_width(D, k):
    """k (D + 1) = 255, 256, 258, 512, 513, 4352 accumulators: below, at and past one trip of the sums' lanes, k = 256"""
    check("width-%d-%d" % (D, k))


# ---- 3: the edges of the block plan ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.N_EDGES)
@pytest.mark.parametrize("D", K.EDGE_DIMS)
def test_n_edges(D, n):
    """one block / two, the 256th block, 256 / 257 / 258 rows a block, a single point, fewer points than clusters"""
    check("edge-%d-%d" % (D, n))


# ---- 4: the edges of k ----------------------------------------------------------------------------------------------------------------------------
def test_k_edges():
    c, l, it = check("k-1")
    assert (l == 0).all()
    c, l, it = check("k-n")
    assert (l == np.arange(7)).all() and c.tobytes() == K.case("k-n")[0].tobytes()
    # k > n: the repairs chain; a donor that was itself repaired is left with -p / 0, the clusters it fed with 0 / 1
    c, l, it = check("k-above-n")
    want_c = K.want("k-above-n")[0]
    assert np.isinf(want_c).any() and (want_c == 0).all(1).any()
    assert (np.isinf(c) == np.isinf(want_c)).all() and (np.sign(c[np.isinf(c)]) == np.sign(want_c[np.isinf(want_c)])).all()
    assert ((c == 0) == (want_c == 0)).all() and (np.isnan(c) == np.isnan(want_c)).all()
    x, s, max_iter, tol = K.case("k-above-n")
    c1, l1, it1 = entry(x, s, 1, tol)      # the first pass alone: 0/0, -p/0, 0/1 (tests/test_kmeans_nd_refs_cpu.py::test_fixture_k_edges)
    first = [t for t in K.want("k-above-n")[3] if t[0] == 0]
    assert np.isnan(c1[0]).all() and (c1[1] == -np.sign(x[first[0][3]]) * np.inf).all() and (c1[2:] == 0).all() and it1 == 1
    assert sorted(l1.tolist()) == [2, 3, 4]


# ---- 5: exact ties ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.TIE_DIMS)
def test_exact_ties(D):
    """integer coordinates.  Two equal starting centroids: the higher index receives nobody and is repaired; lattice points midway between
    two centroids go to the lower index; of a donor's two equally far members the lower index moves"""
    check("tie-centroids-%d" % D)
    c, l, it = check("tie-midway-%d" % D)
    x, s, _, _ = K.case("tie-midway-%d" % D)
    d = np.stack([R.nd_dist(x, cj) for cj in s], 1)
    tied = (d[:, 0] == d[:, 1]) & (d[:, 0] < d[:, 2])
    assert tied.any() and (l[tied] == 0).all()
    x, s, _, _ = K.case("tie-farthest-%d" % D)
    c1, l1, it1 = entry(x, s, 1, 0.0)
    assert l1[7] == 2 and l1[23] == 0 and (l1 == 2).sum() == 1      # rows 7 and 23 are equally far from the donor's mean: row 7 moves
    check("tie-farthest-%d" % D)


# ---- 6: non-finite and overflowing points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", K.NF_DIMS)
def test_non_finite_points(D):
    """a row with a NaN, one with +inf, one with -inf, one of 1e20: label 0 (no distance of theirs is below +inf), centroid 0 NaN or
    infinite exactly where the IEEE sum of its members is, every other centroid bit-identical to the restatement's; once more from a
    start that repairs three clusters out of the one that holds those rows"""
    rows = sorted(K.NF_ROWS.values())
    for tol in ("eps", "tol0"):
        c, l, it = check("nf-%d-data-%s" % (D, tol))
        x = K.case("nf-%d-data-%s" % (D, tol))[0]
        assert (l[rows] == 0).all()
        m = x[l == 0]      # (no repair in this run: centroid 0 is the mean of the points labelled 0)
        for d in range(D):
            col = m[:, d]
            if np.isnan(col).any() or ((col == np.inf).any() and (col == -np.inf).any()):
                assert np.isnan(c[0, d]), (D, d)
            elif np.isinf(col).any():
                assert c[0, d] == col[np.isinf(col)][0], (D, d)
            else:
                assert np.isfinite(c[0, d]), (D, d)
        assert np.isnan(c[0, 0]) and np.isfinite(c[1:]).all() and K.same_bits(c[1:], K.want("nf-%d-data-%s" % (D, tol))[0][1:])
        c, l, it = check("nf-%d-repair-%s" % (D, tol))
        assert (l[rows] == 0).all() and np.isnan(c[0, 0])
    # the repairs' choice shows in the labels of the first pass only (the later passes assign every point afresh): every member of the
    # donor is NaN away from its NaN mean, so the three lowest indices move
    x, s, _, _ = K.case("nf-%d-repair-tol0" % D)
    c1, l1, it1 = entry(x, s, 1, 0.0)
    want_c, want_l, want_it = K.first_pass("nf-%d-repair-tol0" % D)
    assert it1 == want_it == 1 and (l1 == want_l).all() and K.same_bits(c1, want_c)
    assert l1[:3].tolist() == [1, 2, 3] and (l1[3:] == 0).all()


def test_the_repair_ranks_nan_above_inf_above_numbers():
    """a donor whose mean is +inf in one coordinate: its finite members are +inf away, the infinite row NaN away and moves; a donor with
    a 1e20 row: that row alone is +inf away and moves.  Neither is the donor's lowest index."""
    x, s, _, _ = K.case("nf-rank-inf")
    assert entry(x, s, 1, 0.0)[1][K.NF_ROWS["+inf"]] == 1
    check("nf-rank-inf")
    x, s, _, _ = K.case("nf-rank-1e20")
    assert entry(x, s, 1, 0.0)[1][K.NF_ROWS["1e20"]] == 1
    check("nf-rank-1e20")


# ---- 7: limits and optional arguments -------------------------------------------------------------------------------------------------------------
def test_limits_and_optional_outputs():
    x, s, _, _ = K.case("dim-6-data-eps")
    c, l, it = entry(x, s, 0, R.FLT_EPS)
    assert c.tobytes() == s.tobytes() and (l == 0).all() and it == 0      # max_iter = 0: nothing moves
    c, l, it = entry(x, s, 100, 1e10)
    want = R.kmeans_nd(x, s, 100, 1e10)
    assert it == 1 and want[2] == 1 and K.same_bits(c, want[0]) and (l == want[1]).all()      # a huge tolerance: one iteration
    want_c, want_l, want_it, _ = K.want("dim-6-data-eps")
    c, l, it = entry(x, s, 100, R.FLT_EPS, labels=False)
    assert l is None and it == want_it and c.tobytes() == want_c.tobytes()
    c, l, it = entry(x, s, 100, R.FLT_EPS, iterations=False)
    assert it is None and (l == want_l).all() and c.tobytes() == want_c.tobytes()
    c, l, it = entry(x, s, 100, R.FLT_EPS, labels=False, iterations=False)
    assert c.tobytes() == want_c.tobytes()


# ---- 8: memory and repeatability ------------------------------------------------------------------------------------------------------------------
def test_host_and_device_memory_two_runs_and_nothing_left_allocated():
    import torch

    L = capi.load()
    x, s, max_iter, tol = K.case("edge-9-65537")
    want_c, want_l, want_it, _ = K.want("edge-9-65537")
    n, D = x.shape
    xd = torch.from_numpy(np.array(x)).cuda()
    torch.cuda.synchronize()
    live = (C.c_ulonglong * 2)()
    L.cilhip_debug_live_allocations(live)
    before = tuple(live)
    host = [entry(x, s, max_iter, tol) for _ in range(2)]
    dev = []
    for _ in range(2):
        cent = np.array(s, F32, order="C", copy=True)
        lab = torch.full((n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        it = C.c_size_t(UNTOUCHED)
        rc = L.cilhip_kmeans_nd(0, xd.data_ptr(), n, D, capi.MEM_DEVICE, cent.ctypes.data, len(cent), max_iter, C.c_float(tol), lab.data_ptr(), C.byref(it))
        assert rc == capi.OK, L.cilhip_last_error(None)
        dev.append((cent, lab.cpu().numpy().astype(np.int64), int(it.value)))
    L.cilhip_debug_live_allocations(live)
    assert tuple(live) == before
    for c, l, it in host + dev:
        assert c.tobytes() == want_c.tobytes() and l.tobytes() == want_l.tobytes() and it == want_it


# ---- 9: the mirrors -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 16])
def test_python_and_cpp_mirrors(D, tmp_path):
    from cilantro_amd import clustering as cl

    name = "dim-%d-far-eps" % D
    x, s, max_iter, tol = K.case(name)
    want_c, want_l, want_it, _ = K.want(name)
    km = cl.KMeansXf(x).cluster(s, max_iter, tol)
    assert km.getClusterCentroids().tobytes() == want_c.tobytes() and (km.getPointToClusterIndexMap() == want_l).all()
    assert km.getNumberOfPerformedIterations() == want_it
    import torch

    kd = cl.KMeansXf(torch.from_numpy(np.array(x)).cuda()).cluster(np.array(s), max_iter, tol)      # device points, device labels
    assert kd.getClusterCentroids().tobytes() == want_c.tobytes() and (kd.getPointToClusterIndexMap() == want_l).all()
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_kmeans_nd.cpp"), "test_kmeans_nd")
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(x.tobytes() + s.tobytes())
    r = subprocess.run([exe, "run", str(len(x)), str(D), str(len(s)), str(max_iter), src, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
    raw = open(out, "rb").read()
    nc, nl = 4 * s.size, 4 * len(x)
    assert len(raw) == nc + nl + 16
    assert raw[:nc] == km.getClusterCentroids().tobytes()
    assert raw[nc:nc + nl] == km.getPointToClusterIndexMap().astype(np.uint32).tobytes()
    assert np.frombuffer(raw[nc + nl:], np.uint64).tolist() == [want_it, len(np.unique(want_l))]
