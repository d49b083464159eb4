"""CPU: the yardstick of cilhip_kmeans_nd (rule S6) pinned against itself -- the vectorised restatement
(_spectral_refs.kmeans_nd) against a literal point-at-a-time transcription and against order-free sums on lattice clouds -- and, for every
input of tests/test_gpu_kmeans_nd.py, the facts that input was built for (the run's length, the repairs, the exact ties, where the non-finite
rows are), so that no GPU test can pass without having met what it is about."""
import numpy as np
import pytest

import _kmeans_nd_refs as K
import _spectral_refs as R

F32, F64 = np.float32, np.float64


def _names(prefix):
    return [name for name in K.CASES if name.startswith(prefix)]


# ---- 1: literal against vectorised -------------------------------------------------------------------------------------------------------------
def _tiny(D, kind):
    """-> (x, start, max_iter, tol) with n <= 60, k <= 6"""
    x = K.gauss_blobs(60, D, 4, 40 + D)
    if kind == "plain":
        return x, x[:6].copy(), 100, K.EPS
    if kind == "empties":
        s = x[:5].copy()
        s[3] = 500.0
        return x, s, 100, K.EPS
    if kind == "k_above_n":
        x = x[:4]
        return x, np.concatenate([x[:1], x[:1] + 100.0, x[:1] + 200.0, x[:1] + 300.0, x[:1] + 400.0, x[:1] + 500.0]), 8, K.EPS
    if kind == "duplicates":
        return x, x[[0, 1, 0, 1, 2]].copy(), 100, 0.0
    if kind == "lattice":
        x = K.lattice_cloud(60, D, 50 + D, -3, 3)      # plenty of exact ties in both the assignment and the repair
        return x, np.concatenate([x[:3], [np.full(D, 90.0, F32)]]), 100, K.EPS
    x = x.copy()
    x[7, 0], x[21, D - 1], x[33, :] = np.nan, np.inf, 1e20
    if kind == "non_finite":
        return x, x[:4].copy(), 6, K.EPS
    assert kind == "non_finite_repair"
    return x, np.stack([x[0], x[1] + 1000.0, x[2] - 2000.0]), 6, 0.0


@pytest.mark.parametrize("kind", ["plain", "empties", "k_above_n", "duplicates", "lattice", "non_finite", "non_finite_repair"])
@pytest.mark.parametrize("D", K.DIMS)
def test_literal_and_vectorised_restatements_agree(D, kind):
    x, s, max_iter, tol = _tiny(D, kind)
    trace = []
    c, l, it = R.kmeans_nd(x, s, max_iter, tol, trace)
    lc, ll, lit = K.kmeans_nd_literal(x, s, max_iter, tol)
    assert it == lit and (l == ll).all() and K.same_bits(c, lc), (D, kind, it, lit, int((l != ll).sum()))
    if kind in ("empties", "k_above_n", "duplicates", "non_finite_repair"):
        assert trace, (D, kind)
    if kind == "k_above_n":
        assert len(trace) >= 4 and not np.isfinite(c).all()
    if kind in ("non_finite", "non_finite_repair"):
        assert l[7] == 0 and l[21] == 0 and l[33] == 0 and np.isnan(c[0, 0])


def test_the_repair_ranks_nan_above_inf_above_numbers_and_takes_the_lowest_index():
    inf, nan = np.inf, np.nan
    assert R.nd_farthest(np.array([1, 3, 2, 3], F32)) == 1
    assert R.nd_farthest(np.array([1, inf, 2, inf], F32)) == 1
    assert R.nd_farthest(np.array([inf, 3, nan, inf, nan], F32)) == 2
    assert R.nd_farthest(np.array([nan, nan], F32)) == 0
    assert R.nd_farthest(np.array([0, 0, 0], F32)) == 0
    # the order of the entry's key: the distance's bit pattern, the canonical NaN included
    bits = np.array([0.0, 1e-45, 1.0, 3.4e38, inf, nan], F32).view(np.uint32).astype(np.int64)
    assert (np.diff(bits) > 0).all()


# ---- 2: order-free sums ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 5, 16])
def test_on_a_lattice_the_centroids_are_the_rounded_exact_means(D):
    """integer coordinates: every f64 sum is exact, so one pass per cluster in any order gives the restatement's bits (n = 3000: 12 chunks)"""
    x = K.lattice_cloud(3000, D, 60 + D)
    start = x[np.sort(np.unique(x, axis=0, return_index=True)[1])[:5]].copy()      # the first five distinct rows
    for max_iter in (1, 4):
        trace = []
        c, l, it = R.kmeans_nd(x, start, max_iter, 0.0, trace)
        assert 1 <= it <= max_iter and not trace
        # the labels the last centroids were made from: the assignment to the centroids of one update fewer
        prev = R.nd_assign(x, R.kmeans_nd(x, start, it - 1, 0.0)[0])
        order = np.random.default_rng(D).permutation(len(x))
        for j in range(5):
            members = order[prev[order] == j]
            assert len(members)
            assert K.same_bits(c[j], (x[members].astype(F64).sum(0) / len(members)).astype(F32)), (D, max_iter, j)


# ---- 3: what the GPU tests' inputs do ---------------------------------------------------------------------------------------------------------------
def _chunks(n):
    nb = min(256, (n + 255) // 256)
    rows = (n + nb - 1) // nb
    return nb, rows


@pytest.mark.parametrize("name", _names("dim-"))
def test_fixture_every_dimension(name):
    x, s, max_iter, tol = K.case(name)
    c, l, it, trace = K.want(name)
    assert x.shape == (1500, int(name.split("-")[1])) and s.shape[0] == 5
    assert 2 <= it < max_iter and np.isfinite(c).all() and len(np.unique(l)) == 5, (name, it)
    if "-far-" in name:
        assert trace and trace[0][:2] == (0, 4), trace[:2]
    else:
        assert not trace


@pytest.mark.parametrize("name", _names("width-"))
def test_fixture_accumulator_width(name):
    x, s, max_iter, tol = K.case(name)
    c, l, it, trace = K.want(name)
    k, D = s.shape
    assert len(x) == 2000 and it == 3 and (k * (D + 1) > 254)
    assert len(np.unique(l)) == k and np.isfinite(c).all()      # every accumulator holds something


@pytest.mark.parametrize("name", _names("edge-"))
def test_fixture_n_edges(name):
    x, s, max_iter, tol = K.case(name)
    c, l, it, trace = K.want(name)
    n = len(x)
    nb, rows = _chunks(n)
    assert n == int(name.split("-")[2]) and s.shape[0] == 4
    if n >= 255:
        assert it == 3 and not trace and np.isfinite(c).all()
        for lo in range(0, n, rows):      # every chunk of the sums holds every cluster (the last, shorter one included when it has 4 points)
            if min(lo + rows, n) - lo >= 16:
                assert len(np.unique(l[lo:lo + rows])) == 4, (name, lo)
    else:
        assert trace and not np.isfinite(c).all()      # n < k: repeated start rows, chained repairs
    # the block plan's edges are where the issue puts them
    assert _chunks(256) == (1, 256) and _chunks(257) == (2, 129) and _chunks(65536) == (256, 256) and _chunks(65537) == (256, 257)
    assert _chunks(65792) == (256, 257) and _chunks(65793) == (256, 258)


def test_fixture_k_edges():
    c, l, it, trace = K.want("k-1")
    assert (l == 0).all() and it >= 1 and not trace
    c, l, it, trace = K.want("k-n")
    assert (l == np.arange(7)).all() and K.same_bits(c, K.case("k-n")[0]) and not trace
    x, s, max_iter, tol = K.case("k-above-n")
    c, l, it, trace = K.want("k-above-n")
    first = [t for t in trace if t[0] == 0]
    # pass 1: all three points in cluster 0; clusters 1, 2, 3 take them one by one, then cluster 4 takes cluster 1's only member
    assert (R.nd_assign(x, s) == 0).all() and [t[1:3] for t in first] == [(1, 0), (2, 0), (3, 0), (4, 1)] and first[3][3] == first[0][3]
    c1 = R.kmeans_nd(x, s, 1, tol)[0]
    moved = x[first[0][3]]
    assert np.isnan(c1[0]).all() and (c1[1] == -np.sign(moved) * np.inf).all() and (c1[2:] == 0).all()      # 0/0, -p/0, 0/1
    assert it >= 2 and np.isinf(c).any() and (c == 0).all(1).any()


@pytest.mark.parametrize("D", K.TIE_DIMS)
def test_fixture_exact_ties(D):
    # two equal starting centroids
    x, s, max_iter, tol = K.case("tie-centroids-%d" % D)
    c, l, it, trace = K.want("tie-centroids-%d" % D)
    assert s[0].tobytes() == s[2].tobytes() and (R.nd_assign(x, s) != 2).all() and (R.nd_assign(x, s) == 0).any()
    assert trace and trace[0][:2] == (0, 2) and it >= 2
    assert (x == np.round(x)).all()
    # points midway between two centroids
    x, s, max_iter, tol = K.case("tie-midway-%d" % D)
    c, l, it, trace = K.want("tie-midway-%d" % D)
    d = np.stack([R.nd_dist(x, cj) for cj in s], 1)
    tied = (d[:, 0] == d[:, 1]) & (d[:, 0] < d[:, 2])
    assert tied.sum() >= 5 and (l[tied] == 0).all() and it == 1 and (l == 1).any() and (l == 2).any(), (D, int(tied.sum()))
    # two farthest members of the donor, equally far
    x, s, max_iter, tol = K.case("tie-farthest-%d" % D)
    c, l, it, trace = K.want("tie-farthest-%d" % D)
    first = R.nd_assign(x, s)
    members = np.flatnonzero(first == 0)
    assert len(members) == 82 and (first[82:] == 1).all()
    mean = (x[members].astype(F64).sum(0) / 82).astype(F32)
    d = R.nd_dist(x[members], mean)
    assert (mean == 0).all() and members[d == d.max()].tolist() == [7, 23] and d.max() == 900.0
    assert trace[0] == (0, 2, 0, 7) and it >= 2


@pytest.mark.parametrize("name", _names("nf-") )
def test_fixture_non_finite(name):
    x, s, max_iter, tol = K.case(name)
    c, l, it, trace = K.want(name)
    first = R.nd_assign(x, s)
    if name.startswith("nf-rank"):
        row = K.NF_ROWS["+inf" if name.endswith("inf") else "1e20"]
        assert (first == 0).all() and trace[0] == (0, 1, 0, row)      # not the lowest index: the rank decides
        with np.errstate(invalid="ignore", over="ignore"):
            d = R.nd_dist(x, (x.astype(F64).sum(0) / len(x)).astype(F32))
        others = np.delete(d, row)
        if name.endswith("inf"):
            assert np.isnan(d[row]) and (others == np.inf).all()      # NaN above +inf
        else:
            assert d[row] == np.inf and np.isfinite(others).all()     # +inf above every number
        return
    rows = sorted(K.NF_ROWS.values())
    assert np.isnan(x[10, 0]) and x[20, 1] == np.inf and x[30, -1] == -np.inf and (x[40] == F32(1e20)).all()
    assert np.isfinite(np.delete(x, rows, 0)).all() and np.isfinite(s).all()
    assert (first[rows] == 0).all() and (l[rows] == 0).all() and it >= 2
    assert np.isnan(c[0, 0]) and np.isfinite(c[1:]).any()
    if "-repair-" in name:
        # the first repairs take their point out of cluster 0, which holds every non-finite row at that moment
        assert [t[:3] for t in trace[:3]] == [(0, 1, 0), (0, 2, 0), (0, 3, 0)] and (first == 0).all()
        assert [t[3] for t in trace[:3]] == [0, 1, 2]      # every distance from the NaN mean is NaN: the lowest index
        l1 = K.first_pass(name)[1]
        assert l1[:3].tolist() == [1, 2, 3] and (l1[3:] == 0).all()      # (what the GPU test reads the choice from)
    else:
        assert not trace and np.isfinite(c[1:]).all()


def test_every_gpu_input_has_its_facts_asserted_here():
    covered = ("dim-", "width-", "edge-", "k-", "tie-", "nf-")
    assert all(name.startswith(covered) for name in K.CASES)
