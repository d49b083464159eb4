"""What holds cilhip_kmeans_nd (rule S6) at every dimension, size edge and tie:
    kmeans_nd_literal   a second, point-at-a-time transcription of kmeans.hpp:67-194 with the entry's pinned arithmetic; it shares no code
                        with the vectorised restatement (_spectral_refs.kmeans_nd) and is for tiny inputs only
    gauss_blobs, lattice_cloud   the input builders (seeded; on a lattice cloud every f64 sum is exact, so no summation order matters)
    CASES               every input of tests/test_gpu_kmeans_nd.py by name, want(name) its restatement run (computed once, shared, read-only);
                        tests/test_kmeans_nd_refs_cpu.py asserts about each of them what it was built to do"""
import numpy as np

import _spectral_refs as R

F32, F64 = np.float32, np.float64
EPS = R.FLT_EPS


# ---- the literal transcription --------------------------------------------------------------------------------------------------------------
def _rank(d):
    return 2 if d != d else 1 if d == F32(np.inf) else 0


def kmeans_nd_literal(x, centroids, max_iter=100, tol=EPS):
    """kmeans.hpp:67-194 line by line, brute-force branch, one point at a time -> (centroids f32 [k, D], labels, iterations).  Pinned as the
    entry pins it: the distance ((d0 d0 + d1 d1) + d2 d2) + ... in f32; the sums in f64 over chunks of ceil(n / min(256, ceil(n / 256)))
    consecutive points, the chunks added in ascending order; centroid (float)(sum / count); the repair's farthest member with NaN above +inf
    above every number and the lowest index among equals; the largest squared move taken with `>` from 0."""
    x = np.ascontiguousarray(x, F32)
    n, D = x.shape
    k = len(centroids)
    cent = [[F32(v) for v in row] for row in np.asarray(centroids, F32)]
    lab = [0] * n                                                   # :79 resize(): zeros
    tol_sq = F32(tol) * F32(tol)                                    # :70

    def dist(c, p):                                                 # :108, :159
        acc = F32(0)
        for d in range(D):
            df = F32(c[d] - p[d])
            acc = F32(df * df) if d == 0 else F32(acc + F32(df * df))
        return acc

    it = 0
    with np.errstate(all="ignore"):
        while it < max_iter:                                        # :82
            unchanged = True
            for i in range(n):                                      # :101-119
                min_dist, min_ind = F32(np.inf), 0
                for j in range(k):
                    dj = dist(cent[j], x[i])
                    if dj < min_dist:
                        min_dist, min_ind = dj, j
                if lab[i] != min_ind:
                    unchanged = False
                lab[i] = min_ind
            if unchanged and it > 0:                                # :122
                break
            old = [row[:] for row in cent]                          # :123
            nb = min(256, (n + 255) // 256)
            rows = (n + nb - 1) // nb
            sums = [[F64(0)] * D for _ in range(k)]                 # :126-131, f64 in the chunk order
            count = [0] * k
            for b in range(nb):
                part = [[F64(0)] * D for _ in range(k)]
                for i in range(min(b * rows, n), min((b + 1) * rows, n)):
                    for d in range(D):
                        part[lab[i]][d] = part[lab[i]][d] + F64(x[i, d])
                    count[lab[i]] += 1
                for c in range(k):
                    for d in range(D):
                        sums[c][d] = sums[c][d] + part[c][d]
            for i in range(k):                                      # :134-176
                if count[i] != 0:
                    continue
                mx = 0
                for j in range(1, k):                               # :138-141
                    if count[j] > count[mx]:
                        mx = j
                oc = [F32(sums[mx][d] / F64(count[mx])) for d in range(D)]      # :148
                far, far_d = -1, None
                for j in range(n):                                  # :152-169
                    if lab[j] != mx:
                        continue
                    dj = dist(oc, x[j])
                    if far < 0 or _rank(dj) > _rank(far_d) or (_rank(dj) == 0 and _rank(far_d) == 0 and dj > far_d):
                        far, far_d = j, dj
                lab[far] = i                                        # :172-175
                for d in range(D):
                    sums[mx][d] = sums[mx][d] - F64(x[far, d])
                count[mx] -= 1
                count[i] += 1
            for i in range(k):                                      # :179-181
                for d in range(D):
                    cent[i][d] = F32(sums[i][d] / F64(count[i]))
            it += 1                                                 # :183
            if tol > 0:                                             # :186-188
                most = F32(0)
                for i in range(k):
                    sq = dist(cent[i], old[i])
                    if sq > most:
                        most = sq
                if most < tol_sq:
                    break
    return np.array(cent, F32).reshape(k, D), np.array(lab, np.int64), it


# ---- input builders --------------------------------------------------------------------------------------------------------------------------
def gauss_blobs(n, D, k, seed, spread=2.0, sigma=1.0):
    """k Gaussian blobs in D dimensions whose members interleave by index (label = i mod k), so every chunk of the sums holds every
    cluster; the blobs overlap (sigma 1 around centres drawn with deviation `spread`), so Lloyd's loop takes more than a pass"""
    rng = np.random.default_rng(seed)
    centres = spread * rng.standard_normal((k, D))
    return (centres[np.arange(n) % k] + sigma * rng.standard_normal((n, D))).astype(F32)


def lattice_cloud(n, D, seed, lo=-8, hi=8):
    """integer coordinates in [lo, hi]: every sum of them is exact in f64 whatever the order"""
    return np.random.default_rng(seed).integers(lo, hi + 1, (n, D)).astype(F32)


# ---- the GPU tests' inputs ---------------------------------------------------------------------------------------------------------------------
DIMS = list(range(1, 17))
WIDTHS = [(16, 15), (15, 16), (1, 129), (1, 256), (2, 171), (16, 256)]      # (D, k): k (D + 1) = 255, 256, 258, 512, 513, 4352
N_EDGES = [1, 2, 255, 256, 257, 511, 512, 513, 65535, 65536, 65537, 65792, 65793]
EDGE_DIMS = [3, 9]
TIE_DIMS = [2, 5, 16]
NF_DIMS = [2, 6, 16]
NF_ROWS = {"nan": 10, "+inf": 20, "-inf": 30, "1e20": 40}
_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def dim_cloud(D):
    return _once(("dim", D), lambda: gauss_blobs(1500, D, 5, 100 + D))


def edge_cloud(D):
    return _once(("edge", D), lambda: gauss_blobs(65793, D, 4, 300 + D, spread=0.6))


def nf_cloud(D, rows=("nan", "+inf", "-inf", "1e20")):
    """600 points of 4 blobs; row 10 gets a NaN in coordinate 0, row 20 +inf in coordinate 1, row 30 -inf in the last coordinate, row 40 is
    1e20 throughout (its squared distance from any finite centroid overflows f32)"""
    x = gauss_blobs(600, D, 4, 500 + D).copy()
    if "nan" in rows:
        x[NF_ROWS["nan"], 0] = np.nan
    if "+inf" in rows:
        x[NF_ROWS["+inf"], 1] = np.inf
    if "-inf" in rows:
        x[NF_ROWS["-inf"], D - 1] = -np.inf
    if "1e20" in rows:
        x[NF_ROWS["1e20"], :] = 1e20
    return x


def _case_dim(D, start, tol):
    x = dim_cloud(D)
    s = x[:5].copy()
    if start == "far":
        s[4] = 1000.0      # nobody's nearest centroid: cluster 4 is empty after the first pass and gets repaired
    return x, s, 100, tol


def _case_width(D, k):
    x = _once(("width", D), lambda: gauss_blobs(2000, D, 8, 200 + D))
    return x, x[:k].copy(), 3, EPS


def _case_edge(D, n):
    x = edge_cloud(D)[:n]
    return x, x[np.arange(4) % n].copy(), 3, EPS      # (n < 4: repeated rows make the start)


def _case_k1():
    x = gauss_blobs(300, 4, 3, 401)
    return x, x[:1].copy(), 100, EPS


def _case_kn():
    x = gauss_blobs(7, 3, 7, 402)
    return x, x.copy(), 100, EPS


def _case_k_above_n():
    """n = 3, k = 5, D = 5 on integers: every point starts in cluster 0, clusters 1 to 4 are repaired in a chain that empties donors again"""
    x = np.array([[1, 2, 3, 4, 5], [-2, 1, -1, 3, 2], [4, -3, 2, 1, -1]], F32)
    s = np.array([[0, 0, 0, 0, 0], [50, 50, 50, 50, 50], [60, 60, 60, 60, 60], [70, 70, 70, 70, 70], [80, 80, 80, 80, 80]], F32)
    return x, s, 6, EPS


def _case_tie_centroids(D):
    """two equal starting centroids: strict '<' gives cluster 2 (the copy of cluster 0) nobody, and it is repaired"""
    x = lattice_cloud(400, D, 600 + D)
    return x, x[[0, 1, 0, 2]].copy(), 100, EPS


def _case_tie_midway(D):
    """centroids 0 and 1 differ in coordinate 0 only (0 and 4): every lattice point with coordinate 0 equal to 2 is exactly midway"""
    x = lattice_cloud(400, D, 700 + D, -3, 7)
    s = np.zeros((3, D), F32)
    s[1, 0] = 4.0
    s[2, 0], s[2, D - 1] = 2.0, 9.0
    return x, s, 1, EPS      # (one pass: the labels that come out are the tied assignment itself)


def _case_tie_farthest(D):
    """a donor cluster symmetric about the origin (p and -p on integers in [-5, 5]: its mean is exactly 0, squared norms at most 25 D <= 400)
    whose two farthest members, rows 7 and 23, are -+(30, 0, ...): equally far (900), the lower index moves into the empty cluster 2;
    cluster 1 is a small group far away"""
    rng = np.random.default_rng(800 + D)
    half = rng.integers(-5, 6, (40, D)).astype(F32)
    body = np.concatenate([half, -half])[rng.permutation(80)]
    far = np.zeros((1, D), F32)
    far[0, 0] = 30.0
    x = np.concatenate([body[:7], -far, body[7:22], far, body[22:], 200.0 + rng.integers(-2, 3, (20, D)).astype(F32)])
    s = np.zeros((3, D), F32)
    s[1] = 200.0
    s[2] = -5000.0
    return x, s, 100, EPS


def _case_nf(D, start, tol):
    x = nf_cloud(D)
    s = x[:4].copy()
    if start == "repair":
        # every point is nearest to (or, not finite, stays with) centroid 0; clusters 1 to 3 are repaired out of the cluster that holds
        # the non-finite rows
        s = np.stack([x[0], x[1] + 1000.0, x[2] - 2000.0, x[3] + 3000.0]).astype(F32)
    return x, s, 5, tol


def _case_nf_rank(rows):
    """D = 6, a repair whose donor holds `rows`: with +inf alone the donor's mean is +inf in coordinate 1, every finite member is +inf
    away and the infinite row NaN away -- NaN outranks +inf; with 1e20 alone the mean is finite and that row alone is +inf away"""
    x = nf_cloud(6, rows)
    s = np.stack([x[0], x[1] + 1000.0]).astype(F32)
    return x, s, 3, EPS


CASES = {}
for _D in DIMS:
    for _start in ("data", "far"):
        for _tol in (EPS, 0.0):
            CASES["dim-%d-%s-%s" % (_D, _start, "tol0" if _tol == 0.0 else "eps")] = (_case_dim, (_D, _start, _tol))
for _D, _k in WIDTHS:
    CASES["width-%d-%d" % (_D, _k)] = (_case_width, (_D, _k))
for _D in EDGE_DIMS:
    for _n in N_EDGES:
        CASES["edge-%d-%d" % (_D, _n)] = (_case_edge, (_D, _n))
CASES["k-1"] = (_case_k1, ())
CASES["k-n"] = (_case_kn, ())
CASES["k-above-n"] = (_case_k_above_n, ())
for _D in TIE_DIMS:
    CASES["tie-centroids-%d" % _D] = (_case_tie_centroids, (_D,))
    CASES["tie-midway-%d" % _D] = (_case_tie_midway, (_D,))
    CASES["tie-farthest-%d" % _D] = (_case_tie_farthest, (_D,))
for _D in NF_DIMS:
    for _start in ("data", "repair"):
        for _tol in (EPS, 0.0):
            CASES["nf-%d-%s-%s" % (_D, _start, "tol0" if _tol == 0.0 else "eps")] = (_case_nf, (_D, _start, _tol))
CASES["nf-rank-inf"] = (_case_nf_rank, (("+inf",),))
CASES["nf-rank-1e20"] = (_case_nf_rank, (("1e20",),))


def case(name):
    """-> (x f32 [n, D], start f32 [k, D], max_iter, tol); the arrays are shared and read-only"""
    def make():
        f, args = CASES[name]
        x, s, max_iter, tol = f(*args)
        x, s = np.ascontiguousarray(x, F32), np.ascontiguousarray(s, F32)
        x.setflags(write=False)
        s.setflags(write=False)
        return x, s, max_iter, tol
    return _once(("case", name), make)


def want(name):
    """the restatement's run of a case -> (centroids, labels, iterations, trace), computed once and read-only"""
    def make():
        x, s, max_iter, tol = case(name)
        trace = []
        c, l, it = R.kmeans_nd(x, s, max_iter, tol, trace)
        c.setflags(write=False)
        l.setflags(write=False)
        return c, l, it, tuple(trace)
    return _once(("want", name), make)


def first_pass(name):
    """the restatement's run of a case cut after one iteration with tol = 0 -> (centroids, labels, iterations): the labels show which
    points the first pass's repairs moved"""
    def make():
        x, s, _, _ = case(name)
        return R.kmeans_nd(x, s, 1, 0.0)
    return _once(("first", name), make)


def same_bits(a, b):
    """f32 arrays equal as bit patterns, a NaN matching any NaN"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    return bool((nan == np.isnan(b)).all() and (a.view(np.uint32)[~nan] == b.view(np.uint32)[~nan]).all())
