"""The yardstick of the spectral-clustering entries (rules S1-S6 of c_api.h): a numpy restatement.  The reference
itself is not compiled (it needs Eigen and Spectra), so -- as for the warp field -- the eigenpairs come from dense f64 numpy.linalg.eigh of
the same f32-valued matrix and every other rule is transcribed literally from the reference's lines:
    S1  graph_literal (the triplet loop of nearest_neighbor_graph_utilities.hpp:63-118) and graph_csr (the same, vectorised)
    S2  laplacian
    S4  criterion, eigenvalue_bound
    S5  eigengap (spectral_clustering.hpp:46-68)
    S6  kmeans_nd (kmeans.hpp:67-194 in D dimensions with the entry's pinned arithmetic)
and the inputs of the tests (blobs3, blobs5, shells, uniform, blocks7) with what the tests rely on about them."""
import numpy as np

from _meanshift_refs import weights

F32, F64 = np.float32, np.float64
UNITY, IDENTITY, RBF = 0, 1, 2
UNNORMALIZED, NORMALIZED_SYMMETRIC, NORMALIZED_RANDOM_WALK = 0, 1, 2
NONE = 0xFFFFFFFF
FLT_EPS = float(np.finfo(F32).eps)
EPS23 = float(F32(FLT_EPS) ** (F32(2.0) / F32(3.0)))      # Spectra's eps23 for float
TOL = float(F32(1e-7))                                      # spectral_clustering.hpp:202


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def blobs(k, per, sigma=0.05, seed=11):
    """k Gaussian blobs of `per` points, centres on a circle of radius 1.5 lifted along z -> (points f32, planted labels)"""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * np.arange(k) / k
    centres = np.stack([1.5 * np.cos(ang), 1.5 * np.sin(ang), 0.4 * np.arange(k)], 1)
    P = np.concatenate([c + sigma * rng.standard_normal((per, 3)) for c in centres])
    return P.astype(F32), np.repeat(np.arange(k), per)


def shells(seed=0):
    """the reference example's cloud (examples/spectral_clustering.cpp:9-18): two concentric shells, 1500 points of radius 1 and 200 of
    radius 0.3 (directions: normalised points of the cube [-1, 1]^3, as setRandom().normalize() gives), lifted by 4 along z"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-1.0, 1.0, (1700, 3))
    P = v / np.linalg.norm(v, axis=1, keepdims=True) * np.repeat([1.0, 0.3], [1500, 200])[:, None]
    P[:, 2] += 4.0
    return P.astype(F32), np.repeat(np.arange(2), [1500, 200])


def uniform(n=600, seed=5):
    return np.random.default_rng(seed).random((n, 3)).astype(F32), np.zeros(n, np.int64)


def blocks7(per=10000, seed=9):
    """7 unit cubes of `per` points, spaced 3 along x"""
    rng = np.random.default_rng(seed)
    P = rng.random((7 * per, 3))
    P[:, 0] += 3.0 * np.repeat(np.arange(7), per)
    return P.astype(F32), np.repeat(np.arange(7), per)


# name -> (cloud, neighbours, wanted eigenvalues with estimation on / blocks7: off)
INPUTS = {"blobs3": (lambda: blobs(3, 100), 8, 5), "blobs5": (lambda: blobs(5, 67), 6, 6), "shells": (shells, 30, 5), "uniform": (uniform, 10, 4),
          "blocks7": (blocks7, 8, 7)}
_cache = {}


def cloud(name):
    if name not in _cache:
        _cache[name] = INPUTS[name][0]()
    return _cache[name]


def knn_lists(P, k):
    """brute force on the CPU: the k nearest points of every point (itself first) by the engine's pinned f32 distance, equal distances by
    index -> (idx uint32 [n, k], d2 f32 [n, k]).  The GPU tests take their lists from cilhip_knn3f instead."""
    P = np.asarray(P, F32)
    n = len(P)
    idx, d2 = np.empty((n, k), np.uint32), np.empty((n, k), F32)
    for lo in range(0, n, 256):
        d = P[lo:lo + 256, None, :] - P[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.argsort(dd, axis=1, kind="stable")[:, :k]
        idx[lo:lo + 256], d2[lo:lo + 256] = order, np.take_along_axis(dd, order, 1)
    return idx, d2


def lists_to_csr(idx, d2):
    """a padded k-NN list as CSR lists (offsets uint64, idx uint32, d2 f32)"""
    keep = idx != NONE
    off = np.concatenate(([0], np.cumsum(keep.sum(1)))).astype(np.uint64)
    return off, idx[keep].astype(np.uint32), d2[keep].astype(F32)


# ---- S1 -------------------------------------------------------------------------------------------------------------------------
def _entries(idx, d2, offsets):
    """-> (i, position in i's list, j, d2) of every list entry that is not padding"""
    if offsets is None:
        n, k = idx.shape
        i, e = np.repeat(np.arange(n), k), np.tile(np.arange(k), n)
        j, v = idx.reshape(-1).astype(np.int64), d2.reshape(-1)
        keep = j != NONE
        return i[keep], e[keep], j[keep], v[keep]
    counts = np.diff(offsets.astype(np.int64))
    i = np.repeat(np.arange(len(counts)), counts)
    e = np.arange(len(idx)) - np.repeat(offsets[:-1].astype(np.int64), counts)
    return i, e, idx.astype(np.int64), d2


def graph_literal(n, idx, d2, offsets=None, kind=UNITY, sigma=1.0, force_symmetry=False, duplicates=0):
    """the reference's loop, entry by entry: a triplet list summed per (row, column) in list order (setFromTriplets; duplicates=0) or a
    dense matrix assigned in loop order (duplicates=1) -> {(row, column): f32}"""
    i_, e_, j_, v_ = _entries(idx, d2, offsets)
    w_ = weights(kind, sigma, v_)
    M = {}

    def put(r, c, val):
        if duplicates == 0 and (r, c) in M:
            M[(r, c)] = F32(M[(r, c)] + val)
        else:
            M[(r, c)] = F32(val)

    for i, j, val in zip(i_.tolist(), j_.tolist(), w_):      # (ascending i, then ascending position: _entries' order)
        put(j, i, val)
        if force_symmetry:
            put(i, j, val)
    return M


def graph_csr(n, idx, d2, offsets=None, kind=UNITY, sigma=1.0, force_symmetry=False, duplicates=0):
    """the same matrix, vectorised -> (offsets uint64 [n + 1], columns uint32, values f32), columns ascending per row"""
    i, e, j, v = _entries(idx, d2, offsets)
    uniq, inv = np.unique(v, return_inverse=True)      # (the pinned exponential is evaluated once per distinct distance)
    w = weights(kind, sigma, uniq)[inv]
    order_key = i.astype(np.int64) * (1 << 32) + e
    row, col, val, key = j, i, w, order_key
    if force_symmetry:
        # per list entry the triplet (idx, i) comes before (i, idx): a stable sort on the entry's key keeps that
        row, col, val, key = np.concatenate([j, i]), np.concatenate([i, j]), np.concatenate([w, w]), np.concatenate([order_key, order_key])
    order = np.lexsort((key, col, row))
    row, col, val = row[order], col[order], val[order]
    first = np.ones(len(row), bool)
    first[1:] = (row[1:] != row[:-1]) | (col[1:] != col[:-1])
    group = np.cumsum(first) - 1
    start = np.flatnonzero(first)
    pos = np.arange(len(row)) - start[group]
    out = val[start].astype(F32)
    for p in range(1, int(pos.max()) + 1 if len(pos) else 0):
        sel = pos == p
        out[group[sel]] = (out[group[sel]] + val[sel]).astype(F32) if duplicates == 0 else val[sel]
    counts = np.bincount(row[start], minlength=n)
    return np.concatenate(([0], np.cumsum(counts))).astype(np.uint64), col[start].astype(np.uint32), out


def dense(n, off, col, val):
    W = np.zeros((n, n), F64)
    W[np.repeat(np.arange(n), np.diff(off.astype(np.int64))), col.astype(np.int64)] = val.astype(F64)
    return W


# ---- S2 -------------------------------------------------------------------------------------------------------------------------
def laplacian(W, kind):
    """-> (A dense f64, the upper bound of its spectrum, the degrees); the random-walk type is solved in the symmetric form"""
    d = W.sum(1)
    if kind == UNNORMALIZED:
        return np.diag(d) - W, 2.0 * d.max(), d
    s = 1.0 / np.sqrt(d)
    return np.eye(len(W)) - s[:, None] * W * s[None, :], 2.0, d


# ---- S4 -------------------------------------------------------------------------------------------------------------------------
def criterion(theta):
    """Spectra's threshold (HermEigsBase.h:152-167) for float: tol * max(eps^(2/3), |theta|)"""
    return TOL * np.maximum(EPS23, np.abs(np.asarray(theta, F64)))


def eigenvalue_bound(lam_ref, ub):
    """|lambda_out - max(lambda_ref, 0)| <=: the residual criterion (a symmetric Ritz value lies within its residual of an eigenvalue),
    the rounding to f32, the f64 roundoff of an operator of norm <= ub"""
    lam_ref = np.asarray(lam_ref, F64)
    return 1e-7 * np.maximum(FLT_EPS ** (2.0 / 3.0), lam_ref) + 2.0 ** -24 * lam_ref + 1e-11 * ub


# ---- S5 -------------------------------------------------------------------------------------------------------------------------
def eigengap(ev, max_num_clusters):
    """estimateNumberOfClustersEigengap, spectral_clustering.hpp:46-68, line by line in f32"""
    ev = np.asarray(ev, F32)
    min_val, max_val = F32(np.inf), F32(-np.inf)
    max_diff, max_ind = ev[0], 0
    for i in range(len(ev) - 1):
        diff = F32(ev[i + 1] - ev[i])
        if diff > max_diff:
            max_diff, max_ind = diff, i
        if ev[i] < min_val:
            min_val = ev[i]
        if ev[i] > max_val:
            max_val = ev[i]
    if ev[-1] < min_val:
        min_val = ev[-1]
    if ev[-1] > max_val:
        max_val = ev[-1]
    if F32(max_val - min_val) < F32(FLT_EPS):
        return max_num_clusters
    return max_ind + 1


# ---- S6 -------------------------------------------------------------------------------------------------------------------------
def nd_dist(x, c):
    """((d0 d0 + d1 d1) + d2 d2) + ... in f32; x: (n, D), c: (D,) -> (n,)"""
    d = (np.asarray(c, F32)[None, :] - np.asarray(x, F32)).astype(F32)
    acc = d[:, 0] * d[:, 0]
    for t in range(1, d.shape[1]):
        acc = (acc + d[:, t] * d[:, t]).astype(F32)
    return acc


def nd_assign(x, cent):
    best, lab = np.full(len(x), np.inf, F32), np.zeros(len(x), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(len(cent)):      # strict '<' over ascending j
            d = nd_dist(x, cent[j])
            better = d < best
            best[better], lab[better] = d[better], j
    return lab


def nd_sums(x, lab, k):
    """f64 sums and counts in the entry's order: chunks of ceil(n / min(256, ceil(n / 256))) consecutive points, ascending inside a chunk
    (np.cumsum adds sequentially), the chunks' sums added in ascending order"""
    n, D = x.shape
    nb = min(256, (n + 255) // 256)
    rows = (n + nb - 1) // nb
    sums, counts = np.zeros((k, D), F64), np.zeros(k, F64)
    for lo in range(0, n, rows):
        xs, ls = x[lo:lo + rows].astype(F64), lab[lo:lo + rows]
        for c in range(k):
            m = xs[ls == c]
            with np.errstate(invalid="ignore"):      # (+inf and -inf members: NaN, as IEEE has it)
                part = np.cumsum(m, axis=0)[-1] if len(m) else np.zeros(D)
            sums[c] = sums[c] + part
            counts[c] = counts[c] + len(m)
    return sums, counts      # (a block past the end adds an exact zero)


def nd_farthest(dist):
    """the repair's choice among the donor's members, the entry's rule (k_nd_farthest ranks by the distance's bit pattern, then by
    0xFFFFFFFF - index): a NaN distance above +inf above every number, among equal ranks and values the lowest position.  (A distance
    is a sum of squares: never negative.  The reference's `dist > max_dist` from -1, kmeans.hpp:150-167, never accepts a NaN and
    leaves max_dist_ind uninitialised when every distance is one.) -> position in dist"""
    dist = np.asarray(dist, F32)
    rank = np.where(np.isnan(dist), 2, np.where(dist == np.inf, 1, 0))
    top = np.flatnonzero(rank == rank.max())
    if rank.max() == 0:
        top = top[dist[top] == dist[top].max()]
    return int(top[0])


def kmeans_nd(x, centroids, max_iter=100, tol=FLT_EPS, trace=None):
    """KMeans<float, Dynamic>::cluster_ (kmeans.hpp:67-194), brute-force branch -> (centroids, labels, iterations).  trace: a list that
    receives one record per repair, (iteration, empty cluster, donor cluster, moved point)"""
    x = np.ascontiguousarray(x, F32)
    cent = np.ascontiguousarray(centroids, F32).copy()
    k, D = cent.shape
    lab = np.zeros(len(x), np.int64)
    tol_sq = F32(tol) * F32(tol)
    it = 0
    while it < max_iter:
        new = nd_assign(x, cent)
        changed = int((new != lab).sum())
        lab = new
        if changed == 0 and it > 0:
            break
        old = cent.copy()
        sums, counts = nd_sums(x, lab, k)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            for i in range(k):      # :134-176
                if counts[i] != 0:
                    continue
                mx = int(np.argmax(counts))      # (the first largest)
                oc = (sums[mx] / counts[mx]).astype(F32)
                members = np.flatnonzero(lab == mx)
                mi = members[nd_farthest(nd_dist(x[members], oc))]
                if trace is not None:
                    trace.append((it, i, mx, int(mi)))
                lab[mi] = i
                sums[mx] -= x[mi].astype(F64)
                counts[mx] -= 1
                counts[i] += 1      # (:171-175: the point is not added to cluster i's sum)
            cent = (sums / counts[:, None]).astype(F32)
            it += 1
            if tol > 0:
                d = (cent - old).astype(F32)
                sq = d[:, 0] * d[:, 0]
                for t in range(1, D):
                    sq = (sq + d[:, t] * d[:, t]).astype(F32)
                # cilhip_kmeans3f's rule: the largest squared move is taken with `sq > max` from 0, so a NaN move (a centroid that is NaN,
                # or infinite twice running) does not count.  (Eigen's maxCoeff, :187, leaves what a NaN does to the implementation.)
                moved = sq[~np.isnan(sq)]
                if (moved.max() if len(moved) else F32(0)) < tol_sq:
                    break
    return cent, lab, it
