"""numpy restatements of mean-shift clustering over n x dim points (no GPU): the yardsticks of tests/test_gpu_mean_shift_nd.py, pinned
against each other by tests/test_meanshift_nd_refs_cpu.py.

    literal_nd(...)                 the reference's loop as it is written (clustering/mean_shift.hpp:43-112): ball members in
                                    ascending-distance order, an f32 chain `sum += w * p`, `sum *= 1.0f / total_weight`, the serial
                                    first-fit loop, f32 modes
    contract_nd(...)                rules M1-M7 of DESIGN.md section 22 / c_api.h (cilhip_mean_shift_nd): f64 sums slice by slice in
                                    ascending index, one division, NaN for an empty ball, the early stop with iterations = max_iter
    contract_nd(..., reverse=True)  the same with every f64 sum taken in descending index: a stand-in for "another order"
All return dict(shifted, labels, offsets, members, modes, iterations, leaders).  d2 is rule N1 (_knn_nd_refs.d2_matrix); the weights are
those of _meanshift_refs.
"""
from fractions import Fraction

import numpy as np

import _knn_nd_refs as K
import _meanshift_refs as R3

F32 = np.float32
UNITY, IDENTITY, RBF = R3.UNITY, R3.IDENTITY, R3.RBF
MAX_DIM = 16


# ---- the slice plan of rule M3 (csrc/mean_shift_nd_host.hpp; test_meanshift_nd_refs_cpu.py checks the constants against the source) ----
TARGET_BLOCKS, MIN_SLICE, MAX_SLICES, PART_BYTES, TILE = 1024, 512, 256, 64 << 20, 4


def msn_slices(n, n_active):
    nblk = (n_active + 255) // 256
    if nblk == 0:
        return 1
    s = min((TARGET_BLOCKS + nblk - 1) // nblk, n // MIN_SLICE, MAX_SLICES, PART_BYTES // ((MAX_DIM + 1) * 8) // n_active)
    return max(s, 1)


def msn_slice_length(n, slices):
    return ((n + slices - 1) // slices + TILE - 1) // TILE * TILE


def d2_rows(q, p):
    """N1: q (m, dim) against p (n, dim) -> (m, n) float32"""
    return K.d2_matrix(p, q)


def d2_one(a, b):
    return d2_rows(np.asarray(a, F32)[None], np.asarray(b, F32)[None])[0, 0]


def _rows(x, dim=None):
    x = np.ascontiguousarray(x, F32)
    assert x.ndim == 2 and (dim is None or x.shape[1] == dim)
    return x


def first_fit(shifted, cluster_tol):
    """mean_shift.hpp:84-100 -> (labels, leaders): seed i joins the first cluster whose FIRST member is closer than the tolerance"""
    tol_sq = F32(cluster_tol) * F32(cluster_tol)
    s = _rows(shifted)
    leaders, labels = [], np.zeros(s.shape[0], np.int64)
    for i in range(s.shape[0]):
        c = len(leaders)
        if leaders:
            hit = np.nonzero(d2_rows(s[i:i + 1], s[leaders])[0] < tol_sq)[0]
            if hit.size:
                c = int(hit[0])
        if c == len(leaders):
            leaders.append(i)
        labels[i] = c
    return labels, np.asarray(leaders, np.int64)


def _finish(s, cluster_tol, it, f64_modes):
    labels, leaders = first_fit(s, cluster_tol)
    offsets, members = R3.lists_of(labels, len(leaders))
    modes = np.zeros((len(leaders), s.shape[1]), F32)
    with np.errstate(invalid="ignore"):
        for c in range(len(leaders)):
            m = s[members[offsets[c]:offsets[c + 1]]]
            size = offsets[c + 1] - offsets[c]
            if f64_modes:
                modes[c] = (m.astype(np.float64).sum(axis=0) / float(size)).astype(F32)
            else:
                modes[c] = np.cumsum(m, axis=0, dtype=F32)[-1] * (F32(1.0) / F32(size))
    return {"shifted": s, "labels": labels, "offsets": offsets, "members": members, "modes": modes, "iterations": it, "leaders": leaders}


def literal_nd(points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(F32).eps, kind=UNITY, sigma=1.0):
    points = _rows(points)
    dim = points.shape[1]
    s = _rows(points if seeds is None else seeds, dim).copy()
    radius_sq, conv_sq = F32(kernel_radius) * F32(kernel_radius), F32(convergence_tol) * F32(convergence_tol)
    done = np.zeros(s.shape[0], bool)
    it = 0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        while it < max_iter:
            all_converged = True
            todo = np.nonzero(~done)[0]
            dd = d2_rows(s[todo], points) if points.shape[0] else np.zeros((len(todo), 0), F32)
            for row, i in zip(dd, todo):
                idx = np.nonzero(row < radius_sq)[0]
                order = np.argsort(row[idx], kind="stable")      # nanoflann sorts a radius result by distance
                idx = idx[order]
                w = R3.weights(kind, sigma, row[idx])
                if idx.size:      # the f32 chain: acc = acc + w_j * p_j, total = total + w_j, in list order
                    acc = np.cumsum(w[:, None] * points[idx], axis=0, dtype=F32)[-1]
                    total = np.cumsum(w, dtype=F32)[-1]
                else:
                    acc, total = np.zeros(dim, F32), F32(0.0)
                acc = acc * (F32(1.0) / total)
                if d2_one(s[i], acc) < conv_sq:
                    done[i] = True
                else:
                    all_converged = False
                s[i] = acc
            it += 1
            if all_converged:
                break
    return _finish(s, cluster_tol, it, False)


def _seq_sum(x, reverse):
    """sequential f64 sum from 0 along axis 0 (np.cumsum accumulates one element after the other)"""
    if x.shape[0] == 0:
        return np.zeros(x.shape[1:], np.float64)
    return np.cumsum(x[::-1] if reverse else x, axis=0, dtype=np.float64)[-1]


def contract_step_nd(d2_row, points, radius_sq, kind, sigma, slices, reverse=False):
    """rules M1-M3 and M5 for one seed, given its d2 to every point -> the new seed (f32); NaN on every axis for an empty or zero-weight ball"""
    n, dim = points.shape
    length = msn_slice_length(n, slices)
    inside = d2_row < radius_sq
    S_parts, W_parts = [], []
    for y in range(slices):
        lo, hi = min(y * length, n), min((y + 1) * length, n)
        idx = lo + np.nonzero(inside[lo:hi])[0]
        w = R3.weights(kind, sigma, d2_row[idx]).astype(np.float64)
        S_parts.append(_seq_sum(w[:, None] * points[idx].astype(np.float64), reverse))
        W_parts.append(_seq_sum(w[:, None], reverse)[0])
    S, W = _seq_sum(np.array(S_parts).reshape(slices, dim), reverse), _seq_sum(np.array(W_parts).reshape(slices, 1), reverse)[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return (S / W).astype(F32) if W != 0 else np.full(dim, np.nan, F32)


def contract_nd(points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(F32).eps, kind=UNITY, sigma=1.0, reverse=False):
    points = _rows(points)
    n, dim = points.shape
    s = _rows(points if seeds is None else seeds, dim).copy()
    radius_sq, conv_sq = F32(kernel_radius) * F32(kernel_radius), F32(convergence_tol) * F32(convergence_tol)
    active = np.ones(s.shape[0], bool)
    it, nan_any = 0, False
    slices_seen = []
    while it < max_iter and active.any():
        todo = np.nonzero(active)[0]
        slices = msn_slices(n, len(todo))      # M3: once per pass
        slices_seen.append(slices)
        dd = d2_rows(s[todo], points) if n else np.zeros((len(todo), 0), F32)
        for row, i in zip(dd, todo):
            new = contract_step_nd(row, points, radius_sq, kind, sigma, slices, reverse)
            if np.isnan(new[0]):
                nan_any, active[i] = True, False      # M5: never converges, never examined again
            elif d2_one(s[i], new) < conv_sq:
                active[i] = False
            s[i] = new
        it += 1
    if it < max_iter and nan_any:
        it = max_iter
    out = _finish(s, cluster_tol, it, True)
    out["slices"] = slices_seen
    return out


def on_lattice(*arrays):
    """multiples of 2^-10 inside (-8, 8), at most 2^16 rows... of which any f64 sum is exact in any order"""
    return all(a.shape[0] <= 1 << 16 and np.abs(a).max(initial=0) < 8 and np.array_equal(a * 1024, np.round(a * 1024)) for a in arrays)


def contract_lattice(points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(F32).eps, chunk=128):
    """contract_nd for the flat kernel on lattice points (on_lattice): every f64 sum is exact there, so no summation order exists and the
    sums are taken as matrix products -- what makes the large size cases affordable.  Non-finite rows are in no ball and are left out of
    the products.  test_meanshift_nd_refs_cpu.py pins it against contract_nd."""
    points = _rows(points)
    n, dim = points.shape
    fin = np.isfinite(points).all(axis=1)
    assert on_lattice(points[fin])
    p64 = np.where(fin[:, None], points, 0).astype(np.float64)
    s = _rows(points if seeds is None else seeds, dim).copy()
    radius_sq, conv_sq = F32(kernel_radius) * F32(kernel_radius), F32(convergence_tol) * F32(convergence_tol)
    active = np.ones(s.shape[0], bool)
    it, nan_any = 0, False
    slices_seen = []
    while it < max_iter and active.any():
        todo = np.nonzero(active)[0]
        slices_seen.append(msn_slices(n, len(todo)))
        for lo in range(0, len(todo), chunk):
            ids = todo[lo:lo + chunk]
            inside = ((d2_rows(s[ids], points) < radius_sq) if n else np.zeros((len(ids), 0), bool)).astype(np.float64)
            W = inside.sum(axis=1)
            with np.errstate(invalid="ignore", divide="ignore"):
                new = ((inside @ p64) / W[:, None]).astype(F32)
            new[W == 0] = np.nan
            old = s[ids]
            s[ids] = new
            dead = np.isnan(new[:, 0])
            nan_any = nan_any or bool(dead.any())
            with np.errstate(invalid="ignore", over="ignore"):
                conv = np.array([d2_one(o, v) < conv_sq for o, v in zip(old, new)], bool)
            active[ids[dead | conv]] = False
        it += 1
    if it < max_iter and nan_any:
        it = max_iter
    out = _finish(s, cluster_tol, it, True)
    out["slices"] = slices_seen
    return out


def rounds_grouping(shifted, cluster_tol):
    """the parallel formulation of the grouping on a dense d2 matrix -> (labels, leaders, rounds)"""
    s = _rows(shifted)
    n = s.shape[0]
    tol_sq = F32(cluster_tol) * F32(cluster_tol)
    near = d2_rows(s, s) < tol_sq
    np.fill_diagonal(near, False)
    lower = np.tril(near, -1)
    fin = np.isfinite(s).all(axis=1)
    U, leader = fin.copy(), ~fin
    rounds = 0
    while U.any():
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
        labels[i] = rank[i] if leader[i] else rank[hit[0]]
    return labels, idx, rounds


# ---- margins ---------------------------------------------------------------------------------------------------------------------
leader_margin_ok = R3.leader_margin_ok      # (dimension-free already)


def ball_margin_ulps(seeds, points, radius_sq):
    """the smallest distance, in ulps of radius_sq, of any seed-point d2 from radius_sq"""
    d2 = d2_rows(_rows(seeds), _rows(points))
    d2 = d2[np.isfinite(d2)]
    return float(R3.ulps_from(d2, radius_sq).min()) if d2.size else float("inf")


# ---- exact means (the single-step and the mode bounds: DESIGN.md 13.2 carried to dim axes) -----------------------------------------
def exact_step_nd(seed, points, radius_sq, kind, sigma):
    """-> (m, bound, n_ball): the exact rational weighted mean over the pinned f32 weights and the exact ball, per axis as float (the
    Fraction rounded once), and the bound half an f32 ulp of m + 2 (n_ball + 2) 2^-53 sum w |p| / W"""
    points = _rows(points)
    dim = points.shape[1]
    row = d2_rows(np.asarray(seed, F32)[None], points)[0]
    idx = np.nonzero(row < radius_sq)[0]
    w = R3.weights(kind, sigma, row[idx])
    W = sum((Fraction(float(x)) for x in w), Fraction(0))
    m, bound = np.zeros(dim), np.zeros(dim)
    for a in range(dim):
        S = sum((Fraction(float(x)) * Fraction(float(points[j, a])) for x, j in zip(w, idx)), Fraction(0))
        A = sum((Fraction(float(x)) * abs(Fraction(float(points[j, a]))) for x, j in zip(w, idx)), Fraction(0))
        m[a] = float(S / W)
        bound[a] = 0.5 * float(np.spacing(F32(abs(m[a])))) + 2.0 * (len(idx) + 2) * 2.0 ** -53 * float(A / W)
    return m, bound, len(idx)


def exact_mode_nd(shifted, member_idx):
    """-> (m, bound): exact mean of the members' shifted seeds and half an f32 ulp + 2 (size + 2) 2^-53 mean |s|"""
    s = np.asarray(shifted, F32)[member_idx]
    k, dim = s.shape
    m, bound = np.zeros(dim), np.zeros(dim)
    for a in range(dim):
        S = sum((Fraction(float(x)) for x in s[:, a]), Fraction(0))
        A = sum((abs(Fraction(float(x))) for x in s[:, a]), Fraction(0))
        m[a] = float(S / k)
        bound[a] = 0.5 * float(np.spacing(F32(abs(m[a])))) + 2.0 * (k + 2) * 2.0 ** -53 * float(A / k)
    return m, bound


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
quantise = R3.quantise
LATTICE = dict(R3.LATTICE)
UNIT = dict(R3.UNIT)
UNIT_DIMS = (2, 6, 9, 16)


def blob_centres(dim):
    """0, 3 e0 and 3 e1 (dim 1: 0, 3, 6)"""
    c = np.zeros((3, dim))
    if dim == 1:
        c[:, 0] = [0.0, 3.0, 6.0]
    else:
        c[1, 0], c[2, 1] = 3.0, 3.0
    return c


def lattice_sigma(dim):
    return 0.35 * min(1.0, (3.0 / dim) ** 0.5)


def lattice_blobs_nd(dim, per=60, seed=None):
    """three blobs on the 2^-10 lattice, rows interleaved so that every cluster's members are spread over the index range"""
    rng = np.random.default_rng(3 + dim if seed is None else seed)
    p = np.concatenate([c + lattice_sigma(dim) * rng.normal(size=(per, dim)) for c in blob_centres(dim)])
    return quantise(p[rng.permutation(3 * per)])


def lattice_seeds_nd(dim, n=41, seed=None):
    """a seed array of its own: near the blobs and between them, on the lattice"""
    rng = np.random.default_rng(40 + dim if seed is None else seed)
    return quantise(blob_centres(dim)[rng.integers(0, 3, n)] + lattice_sigma(dim) * rng.normal(size=(n, dim)))


def lattice_cloud_nd(dim, n, seed):
    """n lattice points of the three blobs, for the size cases"""
    rng = np.random.default_rng(seed)
    return quantise(blob_centres(dim)[rng.integers(0, 3, n)] + lattice_sigma(dim) * rng.normal(size=(n, dim)))


def unit_blobs_nd(dim, per=100, seed=0):
    """the example's shape in dim dimensions: three N(0, min(1, 3 / dim)) blobs lifted by 10 on the last axis and pushed 2.5 apart along random
    directions; its parameters are UNIT"""
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(3 * per, dim)) * min(1.0, 3.0 / dim) ** 0.5
    p[:, dim - 1] += 10.0
    for c in range(3):
        o = rng.normal(size=dim)
        p[c * per:(c + 1) * per] += 2.5 * o / np.linalg.norm(o)
    return np.ascontiguousarray(p, F32)


def offset_cloud_nd(dim, n=700, seed=5):
    """an unquantised cloud far from the origin (offsets about 100, alternating sign): the single-step fixtures.  The box shrinks with dim
    so that a ball of radius 0.4 keeps a population"""
    rng = np.random.default_rng(seed + dim)
    off = np.array([(100.0 + 3.0 * a) * (-1.0) ** a for a in range(dim)])
    return np.ascontiguousarray(off + rng.random((n, dim)) * (2.0 if dim <= 2 else 0.6 if dim <= 6 else 0.3), F32)


def chain_seeds_nd(dim, n, tol, shuffled=False, seed=6):
    """n seeds 0.9 tol apart along the last axis, in ascending index or shuffled"""
    x = np.arange(n, dtype=np.float64) * (0.9 * tol)
    if shuffled:
        x = x[np.random.default_rng(seed).permutation(n)]
    s = np.zeros((n, dim), F32)
    s[:, dim - 1] = x.astype(F32)
    return s


def collapsed_seeds_nd(dim, n=2000, seed=7):
    """n seeds within 1e-6 of three modes, interleaved"""
    rng = np.random.default_rng(seed)
    modes = blob_centres(dim) * 0.5 + 0.25
    return np.ascontiguousarray(modes[rng.integers(0, 3, n)] + (rng.random((n, dim)) - 0.5) * 1e-6, F32)


def grouping_cases(dim):
    """(name, seeds, cluster_tol) of the grouping-alone cases in dim dimensions"""
    rng = np.random.default_rng(8 + dim)
    dup = rng.random((150, dim)).astype(F32)
    dup = np.concatenate([dup, dup[:60], dup[:20]])[rng.permutation(230)]
    nan = collapsed_seeds_nd(dim, 300)
    nan[0, 0], nan[7, dim - 1], nan[299] = np.nan, np.inf, np.nan
    cases = [("chain", chain_seeds_nd(dim, 200, 0.25), 0.25), ("chain_shuffled", chain_seeds_nd(dim, 200, 0.25, shuffled=True), 0.25),
             ("collapsed", collapsed_seeds_nd(dim), 0.01), ("duplicates", dup, 0.05), ("duplicates_tol0", dup, 0.0), ("nan_seeds", nan, 0.01)]
    for k in (1, 64, 65, 257):
        cases.append((f"uniform_{k}", (rng.random((k, dim)) * 0.5).astype(F32), 0.2 * dim ** 0.5))
    return cases


# The largest |shifted_literal - shifted_contract| over the end-to-end fixtures and the largest |shifted_contract - shifted_reversed|,
# measured by test_meanshift_nd_refs_cpu.py on every run (which asserts that neither is exceeded).
RECORDED_GAP_ND = 2.9e-6
RECORDED_ORDER_GAP_ND = 0.0


def end_to_end_fixtures():
    """(name, points, seeds, parameters)"""
    out = [(f"lattice_{d}", lattice_blobs_nd(d), None, LATTICE) for d in range(1, MAX_DIM + 1)]
    out += [(f"lattice_seeds_{d}", lattice_blobs_nd(d), lattice_seeds_nd(d), LATTICE) for d in range(1, MAX_DIM + 1)]
    out += [(f"unit_{d}", unit_blobs_nd(d), None, UNIT) for d in UNIT_DIMS]
    return out


_FIXTURES = {}
_CACHE = {}


def fixture(name):
    if not _FIXTURES:
        _FIXTURES.update({f[0]: f for f in end_to_end_fixtures()})
    return _FIXTURES[name]


def cached(which, name):
    """literal ("a"), contract ("b") or reversed contract ("r") results of the end-to-end fixtures, computed once per process"""
    key = (which, name)
    if key not in _CACHE:
        _, p, s, prm = fixture(name)
        _CACHE[key] = literal_nd(p, s, **prm) if which == "a" else contract_nd(p, s, reverse=(which == "r"), **prm)
    return _CACHE[key]
