"""Numpy restatement of the robust (MCD) normal-estimation contract, DESIGN.md section 15.1 (test infrastructure; pinned by
test_robust_normal_refs_cpu.py, compared bit for bit with the kernel's decisions by test_gpu_robust_normals.py).

Per point i over its neighbour list L[0..m) (what cilhip_knn3f returns: ascending, L[0] normally the point itself), P_j = x[L[j]]:
    cov(S)      f64 sums of the coordinates over the positions of S, ascending; mean = f32(sum / s); t = P_j - mean in f32; the six
                products in f32; f64 sums of the products; C = sums / (s - 1)
    adj, det    f64, one rounding per operation, in the order written in adj_det()
    q_j         f64, d = f64(P_j - mean) with the difference in f32, in the order written in q_values()
    select(h)   position j is kept iff fewer than h positions l order before it by (q_l, l); a NaN q counts as +inf
    h           min(max(3, llroundf(ratio *f32 f32(m))), m)
    rows        m < 3: NaN; m == 3 or h == m: S = every position, no trials; otherwise trial j = 0..T-1 starts from the 3 distinct positions
                draw3(seed ^ (i << 8 | j), m), takes cov, then R times S = select(h), cov(S); its det replaces the best iff det < best (strict,
                best starts at +inf, a NaN never wins); no winner: NaN row
    result      inlier iff chi <= 0 or q_0 <= f64(chi) * det under the final (mean, C); mask bit j = position j in the final S
Only elementwise float32 / float64 operations (no dot, no einsum: their summation order is not ours), a Python-int splitmix64, and sums
that visit the selected positions one by one -- a row that does not hold position j keeps its sum as it is, it does not add a zero.
Rows are processed side by side (every array below has one entry per row); the arithmetic of a row never sees another row.
"""
import numpy as np

M64 = (1 << 64) - 1


# ---- the sampler: csrc/ransac_sampling.hpp, in Python integers ---------------------------------------------------------------------
def splitmix64(state):
    """-> (value, new state)"""
    state = (state + 0x9E3779B97F4A7C15) & M64
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31), state


def draw3(seed, n):
    """draw_samples(seed, n, 3, 1, out): three distinct indices below n, in the order drawn"""
    st = seed & M64
    pick = []
    for i in range(3):
        z, st = splitmix64(st)
        v = (z * (n - i)) >> 64
        for a in sorted(pick):
            v += 1 if v >= a else 0
        pick.append(v)
    return pick


def trial_seed(seed, row, trial):
    return (seed ^ ((row << 8) | trial)) & M64


def h_of(ratio, m):
    with np.errstate(over="ignore"):
        hf = np.float32(ratio) * np.float32(m)
    if hf >= np.float32(m):
        return int(m)
    return int(min(max(3, int(np.floor(float(hf) + 0.5))), m))      # llroundf: halves away from zero (hf > 0)


# ---- the arithmetic, rows side by side -------------------------------------------------------------------------------------------
def cov(P, sel):
    """P (r, k, 3) f32, sel (r, k) bool -> mean (r, 3) f32, C (r, 6) f64 in the order c00 c01 c02 c11 c12 c22"""
    r, k, _ = P.shape
    s = np.zeros((r, 3), np.float64)
    for j in range(k):
        s = np.where(sel[:, j, None], s + P[:, j, :].astype(np.float64), s)
    cnt = sel.sum(axis=1).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = (s / cnt[:, None]).astype(np.float32)
        cs = np.zeros((r, 6), np.float64)
        for j in range(k):
            t = P[:, j, :] - mean      # f32
            prod = np.stack([t[:, 0] * t[:, 0], t[:, 0] * t[:, 1], t[:, 0] * t[:, 2], t[:, 1] * t[:, 1], t[:, 1] * t[:, 2], t[:, 2] * t[:, 2]], axis=1)
            assert prod.dtype == np.float32
            cs = np.where(sel[:, j, None], cs + prod.astype(np.float64), cs)
        C = cs / (cnt - 1.0)[:, None]
    return mean, C


def adj_det(C):
    """C (r, 6) -> A (r, 6) in the order a00 a01 a02 a11 a12 a22, det (r)"""
    c00, c01, c02, c11, c12, c22 = (C[:, i] for i in range(6))
    with np.errstate(over="ignore", invalid="ignore"):
        a00 = c11 * c22 - c12 * c12
        a01 = c02 * c12 - c01 * c22
        a02 = c01 * c12 - c02 * c11
        a11 = c00 * c22 - c02 * c02
        a12 = c01 * c02 - c00 * c12
        a22 = c00 * c11 - c01 * c01
        det = c00 * a00 + (c01 * a01 + c02 * a02)
    return np.stack([a00, a01, a02, a11, a12, a22], axis=1), det


def q_values(P, mean, A):
    """P (r, k, 3) f32, mean (r, 3) f32, A (r, 6) -> q (r, k) f64"""
    d = (P - mean[:, None, :]).astype(np.float64)
    assert (P - mean[:, None, :]).dtype == np.float32
    d0, d1, d2 = d[:, :, 0], d[:, :, 1], d[:, :, 2]
    a00, a01, a02, a11, a12, a22 = (A[:, i, None] for i in range(6))
    with np.errstate(over="ignore", invalid="ignore"):
        return d0 * (a00 * d0 + (a01 * d1 + a02 * d2)) + (d1 * (a01 * d0 + (a11 * d1 + a12 * d2)) + d2 * (a02 * d0 + (a12 * d1 + a22 * d2)))


def select(q, m, h):
    """q (r, k), m (r), h (r) -> (r, k) bool: the h positions below m that order first by (q, position)"""
    r, k = q.shape
    live = np.arange(k)[None, :] < m[:, None]
    qq = np.where(np.isnan(q), np.inf, q)
    pos = np.arange(k)
    before = np.zeros((r, k), np.int64)
    for l in range(k):
        first = (qq[:, l, None] < qq) | ((qq[:, l, None] == qq) & (l < pos)[None, :])
        before += (first & live[:, l, None]).astype(np.int64)
    return (before < h[:, None]) & live


class Result:
    """per row: m, h, mask (uint32), inlier (uint8), ran (trials were run), won (a covariance was chosen), mean (n, 3) f32, C (n, 6) f64,
    det (n) f64 -- rows without a chosen covariance hold NaN / 0"""


def robust(x, idx, cnt, trials, refinements, ratio=0.75, chi=-1.0, seed=0):
    """x: (n, 3) f32 cloud; idx (n, k) neighbour rows padded with -1; cnt (n) -> Result"""
    x = np.ascontiguousarray(x, np.float32).reshape(-1, 3)
    idx = np.asarray(idx, np.int64)
    m = np.asarray(cnt, np.int64)
    n, k = idx.shape
    assert k <= 32 and len(x) == n
    P = np.where((idx >= 0)[:, :, None], x[np.where(idx >= 0, idx, 0)], np.float32(0))
    h = np.array([h_of(ratio, int(v)) if v >= 3 else 0 for v in range(k + 1)], np.int64)[np.minimum(m, k)]
    live = np.arange(k)[None, :] < m[:, None]
    res = Result()
    res.m, res.h = m, h
    res.ran = (m > 3) & (h < m)
    plain = (m >= 3) & ~res.ran
    sel = np.zeros((n, k), bool)
    mean = np.full((n, 3), np.nan, np.float32)
    C = np.full((n, 6), np.nan)
    won = plain.copy()
    # m == 3 or h == m
    rows = np.nonzero(plain)[0]
    if len(rows):
        sel[rows] = live[rows]
        mean[rows], C[rows] = cov(P[rows], live[rows])
    rows = np.nonzero(res.ran)[0]
    if len(rows):
        Pr, mr, hr = P[rows], m[rows], h[rows]
        best_det = np.full(len(rows), np.inf)
        best_sel = np.zeros((len(rows), k), bool)
        best_mean = np.full((len(rows), 3), np.nan, np.float32)
        best_C = np.full((len(rows), 6), np.nan)
        took = np.zeros(len(rows), bool)
        for t in range(trials):
            s = np.zeros((len(rows), k), bool)
            for a, i in enumerate(rows):
                s[a, draw3(trial_seed(seed, int(i), t), int(mr[a]))] = True
            assert (s.sum(axis=1) == 3).all()
            mu, c = cov(Pr, s)
            for _ in range(refinements):
                s = select(q_values(Pr, mu, adj_det(c)[0]), mr, hr)
                mu, c = cov(Pr, s)
            det = adj_det(c)[1]
            better = det < best_det
            best_det = np.where(better, det, best_det)
            best_sel[better], best_mean[better], best_C[better] = s[better], mu[better], c[better]
            took |= better
        sel[rows], mean[rows], C[rows], won[rows] = np.where(took[:, None], best_sel, False), best_mean, best_C, took
    A, det = adj_det(C)
    q0 = q_values(P[:, :1], mean, A)[:, 0]
    with np.errstate(invalid="ignore", over="ignore"):
        inl = won & ((np.float32(chi) <= 0) | (q0 <= np.float64(np.float32(chi)) * det))
    res.won, res.mean, res.C, res.det = won, mean, C, det
    res.sel = sel
    res.mask = (sel.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint32)
    res.inlier = inl.astype(np.uint8)
    return res


def subset_lists(idx, sel):
    """the rows' selected subsets as neighbour lists for _normal_refs.reference: (idx padded with -1, counts), members in list order"""
    idx = np.asarray(idx, np.int64)
    n, k = idx.shape
    cnt = sel.sum(axis=1).astype(np.int64)
    order = np.argsort(~sel, axis=1, kind="stable")      # selected positions first, in ascending position
    out = np.take_along_axis(idx, order, axis=1)
    out[np.arange(k)[None, :] >= cnt[:, None]] = -1
    return out, cnt


def normals_of(C):
    """unit eigenvector of the smallest eigenvalue of every chosen covariance (f64 eigh; for the statistical CPU test only)"""
    out = np.full((len(C), 3), np.nan)
    ok = np.isfinite(C).all(axis=1)
    c = C[ok]
    M = np.stack([np.stack([c[:, 0], c[:, 1], c[:, 2]], 1), np.stack([c[:, 1], c[:, 3], c[:, 4]], 1), np.stack([c[:, 2], c[:, 4], c[:, 5]], 1)], 1)
    out[ok] = np.linalg.eigh(M)[1][:, :, 0]
    return out


# ---- the clouds --------------------------------------------------------------------------------------------------------------------
def planted_cloud():
    """a jittered 32 x 32 plane patch with 10 % of its points planted 0.5 .. 1.5 lattice steps off the surface -> (cloud f32, planted mask)"""
    rng = np.random.default_rng(3)
    g = np.stack(np.meshgrid(np.arange(32), np.arange(32), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    out = rng.random(1024) < 0.10
    z = rng.normal(0, .01, 1024) + np.where(out, rng.choice([-1., 1.], 1024) * rng.uniform(.5, 1.5, 1024), 0)
    cloud = np.float32(np.concatenate([g + rng.normal(0, .05, g.shape), z[:, None]], 1) / 64)
    return np.ascontiguousarray(cloud), out


def brute_lists(x, k):
    """k-NN lists of a small cloud without the oracle (CPU statistics only): ascending f64 distance, ties by index"""
    x64 = np.asarray(x, np.float64)
    d2 = ((x64[:, None, :] - x64[None, :, :]) ** 2).sum(axis=2)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx.astype(np.int64), np.full(len(x), min(k, len(x)), np.int64)


def tilt_degrees(normals):
    """angle between each normal and the z axis, sign free"""
    nz = np.abs(normals[:, 2]) / np.sqrt((normals * normals).sum(axis=1))
    return np.degrees(np.arccos(np.clip(nz, 0.0, 1.0)))
