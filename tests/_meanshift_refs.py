"""numpy restatements of mean-shift clustering (no GPU): the yardsticks of tests/test_gpu_mean_shift.py, pinned against each other by
tests/test_meanshift_refs_cpu.py.

    literal(...)    (a) the reference's loop as it is written (clustering/mean_shift.hpp:43-112): ball members in ascending-distance order,
                    an f32 chain `sum += w * p`, `sum *= 1.0f / total_weight`, the serial first-fit loop, f32 modes
    contract(...)   (b) the rules of DESIGN.md section 13 / c_api.h (cilhip_mean_shift3f): f64 sums, one division, NaN for an empty ball,
                    the early stop with iterations = max_iter, leaders by the serial first-fit, f64 modes
Both return dict(shifted, labels, offsets, members, modes, iterations, leaders).  d2 is the engine's pinned f32 form in both; the RBF
weights come from oracle.pinned_expf (the device's own sequence of f32 operations).
"""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
UNITY, IDENTITY, RBF = 0, 1, 2


def d2_pinned(q, p):
    """((dx*dx)+(dy*dy))+(dz*dz), every operation rounded to f32; q: (3,) or (m, 3), p: (n, 3) -> (n,) or (m, n)"""
    q, p = np.asarray(q, F32), np.asarray(p, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        if q.ndim == 1:
            d = q[None, :] - p
            return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        d = q[:, None, :] - p[None, :, :]
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def rbf_coeff(sigma):
    return F32(-0.5) / (F32(sigma) * F32(sigma))


def weights(kind, sigma, d2):
    d2 = np.asarray(d2, F32)
    if kind == UNITY:
        return np.ones(d2.shape, F32)
    if kind == IDENTITY:
        return d2.copy()
    from oracle import oracle as orc

    return orc.pinned_expf(rbf_coeff(sigma) * d2).reshape(d2.shape)


def ball(seed, points, radius_sq):
    """-> (indices, d2) of the points inside the seed's ball (strict; NaN compares false: non-finite points and seeds find nothing)"""
    if points.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, F32)
    d2 = d2_pinned(seed, points)
    idx = np.nonzero(d2 < radius_sq)[0]
    return idx, d2[idx]


def first_fit(shifted, cluster_tol):
    """mean_shift.hpp:84-100 -> (labels, leaders): seed i joins the first cluster whose FIRST member is closer than the tolerance"""
    tol_sq = F32(cluster_tol) * F32(cluster_tol)
    s = np.asarray(shifted, F32)
    leaders, labels = [], np.zeros(s.shape[0], np.int64)
    lead_pos = np.zeros((0, 3), F32)
    for i in range(s.shape[0]):
        c = len(leaders)
        if leaders:
            hit = np.nonzero(d2_pinned(s[i], lead_pos) < tol_sq)[0]
            if hit.size:
                c = int(hit[0])
        if c == len(leaders):
            leaders.append(i)
            lead_pos = s[leaders]
        labels[i] = c
    return labels, np.asarray(leaders, np.int64)


def lists_of(labels, k):
    order = np.argsort(labels, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=k))]).astype(np.int64)
    return offsets, order.astype(np.int64)


def literal(points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(F32).eps, kind=UNITY, sigma=1.0):
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    s = np.array(points if seeds is None else seeds, F32).reshape(-1, 3).copy()
    radius_sq, conv_sq = F32(kernel_radius) * F32(kernel_radius), F32(convergence_tol) * F32(convergence_tol)
    done = np.zeros(s.shape[0], bool)
    it = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while it < max_iter:
            all_converged = True
            for i in range(s.shape[0]):
                if done[i]:
                    continue
                idx, d2 = ball(s[i], points, radius_sq)
                order = np.argsort(d2, kind="stable")      # nanoflann sorts a radius result by distance
                idx, d2 = idx[order], d2[order]
                w = weights(kind, sigma, d2)
                acc, total = np.zeros(3, F32), F32(0.0)
                for j, wj in zip(idx, w):
                    acc = acc + wj * points[j]
                    total = total + wj
                acc = acc * (F32(1.0) / total)
                if d2_pinned(s[i], acc[None])[0] < conv_sq:
                    done[i] = True
                else:
                    all_converged = False
                s[i] = acc
            it += 1
            if all_converged:
                break
    labels, leaders = first_fit(s, cluster_tol)
    offsets, members = lists_of(labels, len(leaders))
    modes = np.zeros((len(leaders), 3), F32)
    with np.errstate(invalid="ignore"):
        for c in range(len(leaders)):
            m = np.zeros(3, F32)
            for j in members[offsets[c]:offsets[c + 1]]:
                m = m + s[j]
            modes[c] = m * (F32(1.0) / F32(offsets[c + 1] - offsets[c]))
    return {"shifted": s, "labels": labels, "offsets": offsets, "members": members, "modes": modes, "iterations": it, "leaders": leaders}


def contract_step(seed, points, radius_sq, kind, sigma):
    """rules 1-3 and 5 for one seed -> the new seed (f32); NaN on every axis for an empty or zero-weight ball"""
    idx, d2 = ball(seed, points, radius_sq)
    w = weights(kind, sigma, d2).astype(np.float64)
    S = (w[:, None] * points[idx].astype(np.float64)).sum(axis=0)
    W = w.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        return (S / W).astype(F32) if W != 0 else np.full(3, np.nan, F32)


def contract(points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(F32).eps, kind=UNITY, sigma=1.0):
    points = np.ascontiguousarray(points, F32).reshape(-1, 3)
    s = np.array(points if seeds is None else seeds, F32).reshape(-1, 3).copy()
    radius_sq, conv_sq = F32(kernel_radius) * F32(kernel_radius), F32(convergence_tol) * F32(convergence_tol)
    active = np.ones(s.shape[0], bool)
    it, nan_any = 0, False
    while it < max_iter and active.any():
        for i in np.nonzero(active)[0]:
            new = contract_step(s[i], points, radius_sq, kind, sigma)
            if np.isnan(new[0]):
                nan_any, active[i] = True, False      # rule 5: never converges, never examined again
            elif d2_pinned(s[i], new[None])[0] < conv_sq:
                active[i] = False
            s[i] = new
        it += 1
    if it < max_iter and nan_any:
        it = max_iter
    labels, leaders = first_fit(s, cluster_tol)
    offsets, members = lists_of(labels, len(leaders))
    modes = np.zeros((len(leaders), 3), F32)
    with np.errstate(invalid="ignore"):
        for c in range(len(leaders)):
            modes[c] = (s[members[offsets[c]:offsets[c + 1]]].astype(np.float64).sum(axis=0) / float(offsets[c + 1] - offsets[c])).astype(F32)
    return {"shifted": s, "labels": labels, "offsets": offsets, "members": members, "modes": modes, "iterations": it, "leaders": leaders}


# ---- margins ---------------------------------------------------------------------------------------------------------------------
def leader_margin_ok(shifted, leaders, cluster_tol, lo=0.9, hi=1.1):
    """every seed-leader distance is below lo * tol or above hi * tol (NaN seeds aside)"""
    s = np.asarray(shifted, np.float64)
    fin = np.isfinite(s).all(axis=1)
    lead = s[leaders][np.isfinite(s[leaders]).all(axis=1)]
    d = np.sqrt(((s[fin][:, None, :] - lead[None, :, :]) ** 2).sum(axis=2))
    return bool(((d < lo * cluster_tol) | (d > hi * cluster_tol)).all())


def ulps_from(d2, threshold):
    return np.abs(np.asarray(d2, np.float64) - float(threshold)) / float(np.spacing(F32(threshold)))


def ball_margin_ulps(seeds, points, radius_sq):
    """the smallest distance, in ulps of radius_sq, of any seed-point d2 from radius_sq"""
    d2 = d2_pinned(np.asarray(seeds, F32), points)
    d2 = d2[np.isfinite(d2)]
    return float(ulps_from(d2, radius_sq).min()) if d2.size else math.inf


# ---- exact means (the single-step and the mode bounds) ---------------------------------------------------------------------------
def exact_step(seed, points, radius_sq, kind, sigma):
    """-> (m, bound, n_ball): the exact rational weighted mean over the pinned f32 weights and the exact ball, per axis as float (the
    Fraction rounded once), and the bound half an f32 ulp of m + 2 (n_ball + 2) 2^-53 sum w |p| / W of DESIGN.md 13.2"""
    idx, d2 = ball(seed, points, radius_sq)
    w = weights(kind, sigma, d2)
    W = sum((Fraction(float(x)) for x in w), Fraction(0))
    m, bound = np.zeros(3), np.zeros(3)
    for a in range(3):
        S = sum((Fraction(float(x)) * Fraction(float(points[j, a])) for x, j in zip(w, idx)), Fraction(0))
        A = sum((Fraction(float(x)) * abs(Fraction(float(points[j, a]))) for x, j in zip(w, idx)), Fraction(0))
        m[a] = float(S / W)
        bound[a] = 0.5 * float(np.spacing(F32(abs(m[a])))) + 2.0 * (len(idx) + 2) * 2.0 ** -53 * float(A / W)
    return m, bound, len(idx)


def exact_mode(shifted, member_idx):
    """-> (m, bound): exact mean of the members' shifted seeds and half an f32 ulp + 2 (size + 2) 2^-53 mean |s|"""
    s = np.asarray(shifted, F32)[member_idx]
    k = len(member_idx)
    m, bound = np.zeros(3), np.zeros(3)
    for a in range(3):
        S = sum((Fraction(float(x)) for x in s[:, a]), Fraction(0))
        A = sum((abs(Fraction(float(x))) for x in s[:, a]), Fraction(0))
        m[a] = float(S / k)
        bound[a] = 0.5 * float(np.spacing(F32(abs(m[a])))) + 2.0 * (k + 2) * 2.0 ** -53 * float(A / k)
    return m, bound


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def quantise(x):
    """multiples of 2^-10 inside (-8, 8): every f64 sum of up to 2^16 such numbers is exact in any order"""
    q = np.clip(np.round(np.asarray(x, np.float64) * 1024.0) / 1024.0, -7.9990234375, 7.9990234375)
    return np.ascontiguousarray(q, F32)


LATTICE = {"kernel_radius": 1.0, "max_iter": 100, "cluster_tol": 0.25, "convergence_tol": 1e-4}


def lattice_blobs(per=150, seed=3):
    """three blobs (sigma 0.35, centres 3 apart) on the 2^-10 lattice, interleaved so that every cluster's members are spread over the
    index range"""
    rng = np.random.default_rng(seed)
    centres = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], np.float64)
    p = np.concatenate([c + 0.35 * rng.normal(size=(per, 3)) for c in centres])
    return quantise(p[rng.permutation(3 * per)])


def lattice_seeds(n=41, seed=4):
    """a seed array of its own: near the blobs and between them, on the lattice"""
    rng = np.random.default_rng(seed)
    centres = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0]], np.float64)
    return quantise(centres[rng.integers(0, 3, n)] + 0.5 * rng.normal(size=(n, 3)))


def offset_cloud(n=700, seed=5):
    """an unquantised cloud far from the origin (offset about 100): the single-step fixtures"""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.array([100.0, -97.0, 103.0]) + rng.random((n, 3)) * 2.0, F32)


UNIT = {"kernel_radius": 2.0, "max_iter": 5000, "cluster_tol": 0.2, "convergence_tol": 1e-7}
UNIT_SEED = 0      # (test_meanshift_refs_cpu.py asserts the margin condition for this seed)


def unit_blobs(per=100, seed=UNIT_SEED):
    """the example's shape: three N(0, 1) blobs lifted by 10 along z, pushed 2.5 apart along random directions; its parameters are UNIT"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(3 * per, 3))
    p[:, 2] += 10.0
    for c in range(3):
        o = rng.normal(size=3)
        p[c * per:(c + 1) * per] += 2.5 * o / np.linalg.norm(o)
    return np.ascontiguousarray(p, F32)


def chain_seeds(n, tol, shuffled=False, seed=6):
    """n seeds 0.9 tol apart along x, in ascending index or shuffled"""
    x = np.arange(n, dtype=np.float64) * (0.9 * tol)
    if shuffled:
        x = x[np.random.default_rng(seed).permutation(n)]
    s = np.zeros((n, 3), F32)
    s[:, 0] = x.astype(F32)
    return s


def collapsed_seeds(n=2000, seed=7):
    """n seeds within 1e-6 of three modes, interleaved"""
    rng = np.random.default_rng(seed)
    modes = np.array([[0.5, 0.25, 1.0], [1.5, 0.25, 1.0], [0.5, 1.75, 1.0]], np.float64)
    return np.ascontiguousarray(modes[rng.integers(0, 3, n)] + (rng.random((n, 3)) - 0.5) * 1e-6, F32)


# the largest |shifted_a - shifted_b| over the margin fixtures, measured by test_meanshift_refs_cpu.py (which asserts it is not exceeded):
# 0 on the two lattice fixtures (every sum is exact in f32 too), 2.861e-6 on the unit-scale blobs
RECORDED_GAP = 2.9e-6


def margin_fixtures():
    """(name, points, seeds, parameters) of the end-to-end fixtures"""
    return [("lattice", lattice_blobs(), None, LATTICE), ("lattice_seeds", lattice_blobs(), lattice_seeds(), LATTICE), ("unit", unit_blobs(), None, UNIT)]


_CACHE = {}


def cached(which, name):
    """literal / contract results of the margin fixtures, computed once per process"""
    key = (which, name)
    if key not in _CACHE:
        _, p, s, prm = next(f for f in margin_fixtures() if f[0] == name)
        _CACHE[key] = (literal if which == "a" else contract)(p, s, **prm)
    return _CACHE[key]


def rounds_grouping(shifted, cluster_tol, max_rounds=None):
    """the parallel formulation of the grouping on a dense d2 matrix -> (labels, leaders, rounds): each round, a seed of
    the undecided set U with no lower-index ~-neighbour in U becomes a leader, then every seed of U that is ~ a new leader leaves U;
    labels[i] = rank of the lowest leader ~ i"""
    s = np.asarray(shifted, F32)
    n = s.shape[0]
    tol_sq = F32(cluster_tol) * F32(cluster_tol)
    near = d2_pinned(s, s) < tol_sq
    np.fill_diagonal(near, False)
    lower = np.tril(near, -1)      # lower[i, j]: j < i and j ~ i
    fin = np.isfinite(s).all(axis=1)
    U, leader = fin.copy(), ~fin
    rounds = 0
    while U.any() and (max_rounds is None or rounds < max_rounds):
        new = U & ~(lower & U[None, :]).any(axis=1)
        leader |= new
        U &= ~new
        U &= ~near[:, new].any(axis=1)
        rounds += 1
    idx = np.nonzero(leader)[0]
    rank = np.cumsum(leader) - 1
    labels = np.zeros(n, np.int64)
    for i in range(n):
        hit = idx[near[i, idx]]
        labels[i] = rank[i] if leader[i] else (rank[hit[0]] if hit.size else -1)      # (-1: stopped before the seed was decided)
    return labels, idx, rounds
