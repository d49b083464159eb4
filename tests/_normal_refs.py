"""Plain numpy reference and a-priori error bounds for NormalEstimation3f (test infrastructure; pinned by test_normal_refs_cpu.py).

The product documents the arithmetic of its neighbourhood PCA (knn.hip, c_api.h): the mean is summed in f64 and rounded to f32, the
centred terms and their products are f32 (one rounding each), accumulation and the Jacobi eigen-solve are f64.  With u = 2^-24 and,
per row of m >= 3 neighbours, in float64
    mean, C* = sum (p - mean)(p - mean)^T / (m - 1), eigh -> l0 <= l1 <= l2, v0, tr = l0 + l1 + l2, curvature* = l0 / tr
the covariance the product forms differs from C* by at most (Frobenius norm)
    d_d = spacing(float32(|mean_d|)) / 2            the half-ulp of rounding the mean to f32
    D2  = sum_d d_d^2
    Eb  = (3.0001 u (tr + m/(m-1) D2) + m/(m-1) D2) (1 + 1e-9)
because the covariance about a mean shifted by d is C* + m/(m-1) d d^T, every entry is a sum of products of two f32-rounded
differences rounded once more (relative error (1+u)^3 - 1), and by Cauchy-Schwarz the Frobenius norm of that part is at most
3.0001 u trace; (1 + 1e-9) covers the f64 sums.  What follows from Eb for the returned f32 normal n (taken to f64) and curvature:
    unit length   m >= 3                 | |n| - 1 | <= 4 u
    Rayleigh      m >= 3                 n^T C* n - l0 <= 2 Eb + 8 u l2                       (8 u l2: the f32 rounding of n)
    angle         l1 > l0                |n x v0| <= 2 Eb / (l1 - l0) + 4 u                   (Davis-Kahan; no row left out)
    curvature     tr > 2 sqrt(3) Eb      |curv - l0/tr| <= (1 + sqrt 3) Eb / (tr - sqrt(3) Eb) + 2 u;   tr == 0: curv is NaN (0 / 0)
    view point    m >= 3, view point set n.(vp - p) >= -4.0001 u sum_d |n_d (vp_d - p_d)|     (the f32 dot has four roundings)
    NaN pattern   all rows               normal and curvature NaN exactly where m < 3; elsewhere only the curvature, only where tr == 0
No constant here comes from the code under test.
"""
import numpy as np

U = 2.0 ** -24
SQRT3 = float(np.sqrt(3.0))
CHUNK = 1 << 15


# --------------------------------------------------------------------------------------------------------------------------------
# neighbour lists
# --------------------------------------------------------------------------------------------------------------------------------

def padded_from_csr(offsets, indices, d2=None):
    """CSR lists -> ((n, kmax) rows padded with -1, counts[, (n, kmax) d2 padded with +inf])"""
    offsets = np.asarray(offsets, np.int64)
    cnt = np.diff(offsets)
    n, kmax = len(cnt), max(int(cnt.max()) if len(cnt) else 0, 1)
    col = np.arange(kmax)[None, :]
    live = col < cnt[:, None]
    src = (offsets[:-1, None] + col)[live]
    idx = np.full((n, kmax), -1, np.int64)
    idx[live] = np.asarray(indices, np.int64)[src]
    if d2 is None:
        return idx, cnt
    dd = np.full((n, kmax), np.inf, np.float32)
    dd[live] = np.asarray(d2, np.float32)[src]
    return idx, cnt, dd


def rows_with_equal_distances(d2, cnt):
    """rows of an ascending (n, k) distance table (first cnt entries live) that hold two exactly equal distances"""
    d2 = np.asarray(d2, np.float32)
    cnt = np.asarray(cnt, np.int64)
    if d2.shape[1] < 2:
        return np.zeros(len(d2), bool)
    live = np.arange(1, d2.shape[1])[None, :] < cnt[:, None]
    return ((d2[:, 1:] == d2[:, :-1]) & live).any(axis=1)


# --------------------------------------------------------------------------------------------------------------------------------
# reference
# --------------------------------------------------------------------------------------------------------------------------------

class Reference:
    """per row: m, mean (n,3), C (n,3,3), lam (n,3) ascending, v0 (n,3), tr, curv, Eb -- float64; rows with m < 3 hold NaN"""

    def __init__(self, n):
        self.m = np.zeros(n, np.int64)
        self.mean = np.full((n, 3), np.nan)
        self.C = np.full((n, 3, 3), np.nan)
        self.lam = np.full((n, 3), np.nan)
        self.v0 = np.full((n, 3), np.nan)
        self.tr = np.full(n, np.nan)
        self.curv = np.full(n, np.nan)
        self.Eb = np.full(n, np.nan)


def covariance_bound(mean, tr, m):
    """Eb of the module docstring"""
    d = np.spacing(np.abs(mean).astype(np.float32)).astype(np.float64) / 2.0
    D2 = (d * d).sum(axis=-1)
    f = m / (m - 1.0)
    return (3.0001 * U * (tr + f * D2) + f * D2) * (1.0 + 1e-9)


def reference(x, idx, cnt):
    """x: f32 cloud; idx: (n, k) neighbour rows padded with -1; cnt: neighbours per row -> Reference"""
    x64 = np.asarray(x, np.float32).reshape(-1, 3).astype(np.float64)
    idx = np.asarray(idx, np.int64)
    cnt = np.asarray(cnt, np.int64)
    n, k = idx.shape
    live_all = np.arange(k)[None, :] < cnt[:, None]
    assert np.array_equal(live_all, idx >= 0), "rows must be padded with -1 behind their count"
    R = Reference(n)
    R.m[:] = cnt
    for a in range(0, n, CHUNK):
        b = min(a + CHUNK, n)
        ok = cnt[a:b] >= 3
        if not ok.any():
            continue
        rows = a + np.nonzero(ok)[0]
        live = live_all[rows][:, :, None]
        m = cnt[rows].astype(np.float64)
        P = np.where(live, x64[np.where(idx[rows] >= 0, idx[rows], 0)], 0.0)
        mean = P.sum(axis=1) / m[:, None]
        d = np.where(live, P - mean[:, None, :], 0.0)
        C = np.einsum("nki,nkj->nij", d, d) / (m - 1.0)[:, None, None]
        lam, vec = np.linalg.eigh(C)
        R.mean[rows], R.C[rows], R.lam[rows], R.v0[rows] = mean, C, lam, vec[:, :, 0]
        tr = lam.sum(axis=1)
        R.tr[rows] = tr
        with np.errstate(divide="ignore", invalid="ignore"):
            R.curv[rows] = lam[:, 0] / tr
        R.Eb[rows] = covariance_bound(mean, tr, m)
    return R


def reference_csr(x, offsets, indices):
    idx, cnt = padded_from_csr(offsets, indices)
    return reference(x, idx, cnt)


# --------------------------------------------------------------------------------------------------------------------------------
# checks
# --------------------------------------------------------------------------------------------------------------------------------

def _tally(rows, value, bound, keep=5):
    """value <= bound on `rows` (indices); a NaN on either side is a violation"""
    value, bound = np.asarray(value, np.float64), np.asarray(bound, np.float64)
    good = value <= bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(value > 0, value / bound, 0.0)
    ratio = np.where(good, ratio, np.where(np.isnan(ratio), np.inf, ratio))
    bad = rows[~good]
    return {"rows": int(len(rows)), "violations": int(len(bad)), "worst ratio": float(ratio.max()) if len(rows) else 0.0,
            "first": [int(i) for i in bad[:keep]]}


def _flags(rows_bad, n_rows, keep=5):
    bad = np.nonzero(rows_bad)[0]
    return {"rows": int(n_rows), "violations": int(len(bad)), "worst ratio": float("inf") if len(bad) else 0.0, "first": [int(i) for i in bad[:keep]]}


def check(R, normals, curvature=None, points=None, view_point=None):
    """The checks of the module docstring on a Reference and the returned f32 normals (n, 3) / curvature (n) or None.
    points + view_point: the queries and the view point the normals were oriented towards (None: sign free).
    -> {check: {"rows", "violations", "worst ratio" (value / bound), "first" (violating rows)}}"""
    nrm = np.asarray(normals, np.float32).reshape(-1, 3).astype(np.float64)
    n = len(nrm)
    assert n == len(R.m)
    valid = np.nonzero(R.m >= 3)[0]
    nv, C, lam, Eb = nrm[valid], R.C[valid], R.lam[valid], R.Eb[valid]
    out = {}
    out["unit length"] = _tally(valid, np.abs(np.sqrt((nv * nv).sum(axis=1)) - 1.0), np.full(len(valid), 4 * U))
    ray = np.einsum("ni,nij,nj->n", nv, C, nv) - lam[:, 0]
    out["rayleigh"] = _tally(valid, ray, 2 * Eb + 8 * U * lam[:, 2])
    gap = lam[:, 1] - lam[:, 0]
    g = gap > 0
    cr = np.cross(nv[g], R.v0[valid][g])
    out["angle"] = _tally(valid[g], np.sqrt((cr * cr).sum(axis=1)), 2 * Eb[g] / gap[g] + 4 * U)
    if curvature is not None:
        cur = np.asarray(curvature, np.float32).reshape(-1).astype(np.float64)
        tr = R.tr[valid]
        c = tr > 2 * SQRT3 * Eb
        out["curvature"] = _tally(valid[c], np.abs(cur[valid][c] - R.curv[valid][c]), (1 + SQRT3) * Eb[c] / (tr[c] - SQRT3 * Eb[c]) + 2 * U)
        z = valid[tr == 0]
        out["curvature where trace == 0"] = _flags(~np.isnan(cur[z]), len(z))
        out["curvature where trace == 0"]["first"] = [int(z[i]) for i in out["curvature where trace == 0"]["first"]]
    if view_point is not None:
        vp = np.asarray(view_point, np.float32).astype(np.float64).reshape(3)
        t = nv * (vp[None, :] - np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)[valid])
        out["view point"] = _tally(valid, -t.sum(axis=1), 4.0001 * U * np.abs(t).sum(axis=1))
    few = R.m < 3
    nan_n = np.isnan(nrm)
    bad = np.where(few, ~nan_n.all(axis=1), nan_n.any(axis=1))
    if curvature is not None:
        nan_c = np.isnan(cur)
        zero_tr = np.zeros(n, bool)
        zero_tr[valid] = R.tr[valid] == 0
        bad |= np.where(few, ~nan_c, nan_c & ~zero_tr)
    out["nan pattern"] = _flags(bad, n)
    return out


def violations(res):
    """[(check, violations, worst ratio, first rows)] of the checks that do not hold"""
    return [(name, r["violations"], r["worst ratio"], r["first"]) for name, r in res.items() if r["violations"]]


def summary(R, res, d2=None, cnt=None):
    """what a test reports per case"""
    s = {"rows checked": int(len(R.m)), "rows with m < 3": int((R.m < 3).sum())}
    if d2 is not None:
        s["rows whose list holds equal distances"] = int(rows_with_equal_distances(d2, cnt).sum())
    s["checks"] = {name: {"rows": r["rows"], "violations": r["violations"], "worst ratio": r["worst ratio"]} for name, r in res.items()}
    return s


# --------------------------------------------------------------------------------------------------------------------------------
# the clouds the CPU and GPU tests share
# --------------------------------------------------------------------------------------------------------------------------------

FRAME_OFFSET = (1e3, -250.0, 37.0)
EDGE_SIZES = (3, 4, 63, 64, 65, 255, 256, 257, 513)
EDGE_KS = (3, 10, 32)
H = 2.0 ** -6


def frame():
    import os

    f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_full.npz"))
    return np.ascontiguousarray(f["p1"], np.float32)


def moved(x, offset):
    return np.ascontiguousarray((np.asarray(x, np.float32).astype(np.float64) + np.asarray(offset, np.float64)).astype(np.float32))


def edge_cloud(p1, n):
    """the first n points of the frame after a fixed shuffle"""
    return np.ascontiguousarray(p1[np.random.default_rng(5).permutation(len(p1))[:n]])


def edge_radius_sq(d2_3, cnt_3):
    """a squared radius that leaves some rows of a cloud under 3 members: the median squared distance to the third neighbour (strict <)"""
    assert (cnt_3 == 3).all()
    return np.float32(np.median(d2_3[:, 2]))


def plane_lattice():
    """32 x 32 lattice of spacing 2^-6 in the plane z = 4096.5, x and y offset by 4096 (dyadic: the f32 inputs are exact)"""
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    x = np.concatenate([g * H + 4096.0, np.full((len(g), 1), 4096.5)], axis=1)
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return np.ascontiguousarray(x.astype(np.float32))


def line_cloud():
    """40 points t (1, 1, 2) 2^-6 + (8, -8, 4)"""
    t = np.arange(40, dtype=np.float64)[:, None]
    x = t * np.array([1.0, 1.0, 2.0]) * H + np.array([8.0, -8.0, 4.0])
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    return np.ascontiguousarray(x.astype(np.float32))


def repeated_points():
    """16 copies of one point followed by 16 copies of another"""
    return np.ascontiguousarray(np.concatenate([np.tile(np.float32([0.3, -1.7, 2.9]), (16, 1)), np.tile(np.float32([5.25, 0.1, -3.3]), (16, 1))]))


def doubled_frame(p1):
    """the frame's first 5000 points, each doubled"""
    return np.ascontiguousarray(np.repeat(p1[:5000], 2, axis=0))


STRICT_R2 = np.float32(9.0 * 2.0 ** -14)      # the squared z spacing of strict_lattice, exactly


def strict_lattice():
    """g (h, h, 1.5 h) + (8, -8, 4), h = 2^-6, g in 12 x 12 x 6 -> (cloud, interior mask)"""
    g = np.stack(np.meshgrid(np.arange(12), np.arange(12), np.arange(6), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    x = g * np.array([H, H, 1.5 * H]) + np.array([8.0, -8.0, 4.0])
    assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
    interior = ((g[:, :2] >= 1) & (g[:, :2] <= 10)).all(axis=1) & (g[:, 2] >= 1) & (g[:, 2] <= 4)
    return np.ascontiguousarray(x.astype(np.float32)), interior


# --------------------------------------------------------------------------------------------------------------------------------
# cases: a cloud, the call under test and the oracle's neighbour lists for it
# --------------------------------------------------------------------------------------------------------------------------------

FRAME_R2 = np.float32(0.004) * np.float32(0.004)      # what NormalEstimation3f makes of a radius of 0.004
RADIUS_LIST_K = 64                                   # list length of the k-NN-in-radius route to a radius neighbourhood (the oracle's longest)


def oracle_lists(orc, x, call):
    """call: ("knn", k, r2) or ("radius", r2) -> (idx (n, k) padded with -1, counts, d2) from the CPU oracle, never from the product.
    A radius neighbourhood of a large cloud is listed as a k-NN-in-radius search with a k above the largest count."""
    if call[0] == "knn":
        idx, d2, cnt = orc.knn_batch(orc.KDTree(x), x, call[1], call[2])
        return idx, cnt.astype(np.int64), d2
    if len(x) > 4000:
        idx, d2, cnt = orc.knn_batch(orc.KDTree(x), x, RADIUS_LIST_K, call[1])
        assert cnt.max() < RADIUS_LIST_K, int(cnt.max())
        return idx, cnt.astype(np.int64), d2
    off, ind, dd = orc.radius_search(x, x, call[1])
    return padded_from_csr(off, ind, dd)


def frame_cases(p1):
    """(tag, cloud, call, view point): section (a) -- the view point is the sensor"""
    origin = np.zeros(3, np.float32)
    pm = moved(p1, FRAME_OFFSET)
    return (("knn10", p1, ("knn", 10, np.inf), origin),
            ("knn32", p1, ("knn", 32, np.inf), origin),
            ("knn12_in_radius", p1, ("knn", 12, FRAME_R2), origin),
            ("radius", p1, ("radius", FRAME_R2), origin),
            ("knn10_no_view_point", p1, ("knn", 10, np.inf), None),
            ("knn10_moved", pm, ("knn", 10, np.inf), np.asarray(FRAME_OFFSET, np.float32)))


def edge_cases(orc, p1):
    """section (b): n points, k in EDGE_KS (k > n: m = n), plain k-NN, k-NN inside a radius that leaves some rows under 3 members,
    and that radius alone"""
    for n in EDGE_SIZES:
        x = edge_cloud(p1, n)
        _, d2_3, cnt_3 = orc.knn_batch(orc.KDTree(x), x, 3, np.inf)
        r2 = edge_radius_sq(d2_3, cnt_3)
        vp = np.float32([0.1, -0.2, 0.05])
        for k in EDGE_KS:
            yield f"n={n}/knn {k}", x, ("knn", k, np.inf), vp
            yield f"n={n}/knn {k} in radius", x, ("knn", k, r2), vp if k != 10 else None
        yield f"n={n}/radius", x, ("radius", r2), vp


def degenerate_cases(p1):
    """section (c)"""
    lat = plane_lattice()
    return (("plane lattice, view point in the plane", lat, ("knn", 9, np.inf), np.float32([4096.25, 4096.25, 4096.5])),
            ("plane lattice, no view point", lat, ("knn", 9, np.inf), None),
            ("line", line_cloud(), ("knn", 5, np.inf), np.float32([0.0, 0.0, 0.0])),
            ("two repeated points", repeated_points(), ("knn", 8, np.inf), np.float32([0.0, 0.0, 0.0])),
            ("doubled frame points", doubled_frame(p1), ("knn", 6, np.inf), np.zeros(3, np.float32)))


def strict_cases():
    """section (d): the squared z spacing itself (strict <: own layer only) and the next f32 above it"""
    x, _ = strict_lattice()
    up = np.nextafter(STRICT_R2, np.float32(1.0))
    vp = np.float32([8.0, -8.0, 40.0])
    return (("radius at the spacing", x, ("radius", STRICT_R2), vp), ("radius one ulp above", x, ("radius", up), vp),
            ("knn 32 in radius at the spacing", x, ("knn", 32, STRICT_R2), vp), ("knn 32 in radius one ulp above", x, ("knn", 32, up), vp))
