"""The yardstick of DESIGN.md section 23 (cilhip_connected_components_nd, rules C1-C5) in numpy float32: the edges from rule N1
(_knn_nd_refs.d2_matrix) in row blocks, the clauses of C2 with the dot product's fold written out, and the tail of _cc_refs (union_find,
finish).  Also numpy mirrors of the host plan of csrc/components_nd_host.hpp (the order-preserving key, R, the prune rule) and the
fixtures the CPU and GPU tests share.  Nothing here runs on a device or calls the library."""
import numpy as np

import _cc_refs as R3
from _knn_nd_refs import d2_matrix

F32 = np.float32
TILE = 256      # CCN_TILE of csrc/components_nd_host.hpp (tests/test_ccn_refs_cpu.py checks that the source still says so)
Clauses = R3.Clauses      # normals: n x dim here


# ---- C1: the pairs inside the radius ----------------------------------------------------------------------------------------------
def pairs(p, radius_sq, block=512):
    """every pair i > j with d2(i, j) < radius_sq (strict; NaN and +inf never are) -> (i, j, d2)"""
    p = np.ascontiguousarray(p, F32)
    n = p.shape[0]
    oi, oj, od = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, F32)]
    if radius_sq > 0 and n > 1:
        cols = np.arange(n)
        for r0 in range(0, n, block):
            d = d2_matrix(p, p[r0:r0 + block])      # [rows of the block, n]
            with np.errstate(invalid="ignore"):
                hit = (d < F32(radius_sq)) & (cols[None, :] < (r0 + np.arange(d.shape[0]))[:, None])
            a, b = np.nonzero(hit)
            oi.append(a + r0); oj.append(b); od.append(d[a, b])
    return np.concatenate(oi), np.concatenate(oj), np.concatenate(od)


# ---- C2: the clauses --------------------------------------------------------------------------------------------------------------
def dot_fold(a, b):
    """c_0 + (c_1 + (... + c_{dim-1})), c_a = a_a * b_a: every product and sum rounded to f32, folded from the last axis"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        r = a[..., -1] * b[..., -1]
        for d in range(a.shape[-1] - 2, -1, -1):
            r = a[..., d] * b[..., d] + r
    assert r.dtype == F32
    return r


def pair_angle(nrm, i, j):
    with np.errstate(invalid="ignore"):
        return np.arccos(dot_fold(nrm[i], nrm[j]).astype(np.float64)).astype(F32)


def color_d2(col, i, j):
    d = col[i] - col[j]
    return R3.dot_pinned(d, d)


def similar(c, i, j, d2):
    i, j, d2 = np.asarray(i), np.asarray(j), np.asarray(d2, F32)
    ok = np.ones(i.shape, bool)
    if c.max_distance is not None:
        ok &= d2 < c.max_distance
    if c.color_thresh is not None:
        ok &= color_d2(c.colors, i, j) < c.color_thresh * c.color_thresh
    if c.max_angle is not None:
        v, lim = R3.folded_angle(c, pair_angle(c.normals, i, j))
        with np.errstate(invalid="ignore"):
            ok &= (v <= lim) if c.angle_inclusive else (v < lim)
    return ok


_PAIRS = {}


def cached_pairs(p, radius_sq):
    key = (id(p), float(radius_sq))      # the pair list of a fixture is computed once and shared by every test that needs it
    if key not in _PAIRS or _PAIRS[key][0] is not p:
        if len(_PAIRS) > 64:
            _PAIRS.clear()
        _PAIRS[key] = (p, pairs(p, radius_sq))
    return _PAIRS[key][1]


def roots(p, radius_sq, clauses=None):
    i, j, d2 = cached_pairs(p, radius_sq)
    ok = similar(clauses or Clauses(), i, j, d2)
    return R3.union_find(p.shape[0], i[ok], j[ok])


def components(p, radius_sq, clauses=None, seeds=None, min_segment_size=1, max_segment_size=None):
    """-> (labels, offsets, members), int64, as the entry returns them"""
    return R3.finish(p.shape[0], roots(p, radius_sq, clauses), seeds, min_segment_size, max_segment_size)


def margins(p, radius_sq, clauses=None, ulps=4):
    """how many decisions of a fixture sit within `ulps` of their threshold -> dict(radius, distance, colour, angle)"""
    i, j, d2 = pairs(p, F32(radius_sq) * F32(1.001))
    out = {"radius": int((R3.ulp_distance(d2, np.full(d2.shape, radius_sq, F32)) <= ulps).sum()), "distance": 0, "colour": 0, "angle": 0}
    inside = d2 < F32(radius_sq)
    i, j, d2 = i[inside], j[inside], d2[inside]
    c = clauses or Clauses()
    if c.max_distance is not None:
        out["distance"] = int((R3.ulp_distance(d2, np.full(d2.shape, c.max_distance, F32)) <= ulps).sum())
    if c.color_thresh is not None:
        cd = color_d2(c.colors, i, j)
        out["colour"] = int((R3.ulp_distance(cd, np.full(cd.shape, c.color_thresh * c.color_thresh, F32)) <= ulps).sum())
    if c.max_angle is not None:
        v, lim = R3.folded_angle(c, pair_angle(c.normals, i, j))
        fin = np.isfinite(v) & (v > 0)
        out["angle"] = int((R3.ulp_distance(v[fin], np.full(int(fin.sum()), lim, F32)) <= ulps).sum())
    return out


# ---- the host plan, restated ------------------------------------------------------------------------------------------------------
def key(v):
    """the order-preserving integer image of a float: ascending keys = ascending floats, -0 before +0"""
    u = np.ascontiguousarray(v, F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def prune_radius(radius_sq):
    """R: the smallest f32 with fl(R * R) >= radius_sq, by bisection over the bit pattern"""
    r2 = F32(radius_sq)
    lo, hi = 0, 0x7F7FFFFF
    with np.errstate(over="ignore", under="ignore"):
        while hi - lo > 1:
            mid = (lo + hi) // 2
            r = np.array([mid], np.uint32).view(F32)[0]
            if r * r >= r2:
                hi = mid
            else:
                lo = mid
    return np.array([hi], np.uint32).view(F32)[0]


def pick_axis(p):
    """the axis of largest extent over the rows that are finite on every axis, lowest axis on ties"""
    fin = p[np.isfinite(p).all(axis=1)].astype(np.float64)
    return int(np.argmax(fin.max(axis=0) - fin.min(axis=0)))      # (argmax returns the first maximum)


def sweep_order(p, axis):
    """form 2's stream: the finite rows sorted stably by the key of coordinate `axis` -> original indices"""
    fin = np.nonzero(np.isfinite(p).all(axis=1))[0]
    return fin[np.argsort(key(p[fin, axis]), kind="stable")]


def first_columns(coord_sorted, R, tile=TILE):
    """first[I]: the first column tile row tile I meets, by the literal scan of the rule (skip while fl(min_a(I) - max_a(J)) >= R)"""
    c = np.asarray(coord_sorted, F32)
    tiles = (len(c) + tile - 1) // tile
    tmin = c[::tile]
    tmax = np.array([c[min((t + 1) * tile, len(c)) - 1] for t in range(tiles)], F32)
    first = np.zeros(tiles, np.int64)
    with np.errstate(over="ignore"):
        for t in range(tiles):
            j = 0
            while j < t and F32(tmin[t] - tmax[j]) >= R:
                j += 1
            first[t] = j
    return first


# ---- fixtures (computed once per process) -----------------------------------------------------------------------------------------
_CACHE = {}


def _once(name, make):
    if name not in _CACHE:
        _CACHE[name] = make()
    return _CACHE[name]


def radius_for(p, q):
    """a radius_sq near the q-quantile of the nearest-neighbour d2 that no pair of the cloud decides closely: the middle of the widest gap
    between the pair distances within 1 % of that quantile (tests/test_ccn_refs_cpu.py asserts the margin every fixture ends up with)"""
    p = np.ascontiguousarray(p, F32)
    if len(p) < 2:
        return F32(1.0)
    d = d2_matrix(p, p)
    np.fill_diagonal(d, np.inf)
    d = np.where(np.isnan(d), np.inf, d)
    nn = np.sort(d.min(axis=1).astype(np.float64))
    nn = nn[np.isfinite(nn)]
    target = nn[min(int(q * len(nn)), len(nn) - 1)]
    near = np.unique(d[(d > 0.99 * target) & (d < 1.01 * target)].astype(np.float64))
    edges = np.concatenate([[0.99 * target], near, [1.01 * target]])
    k = int(np.argmax(np.diff(edges)))
    return F32(0.5 * (edges[k] + edges[k + 1]))


def blobs(dim, n=1500, seed=0, centres=4, spread=6.0):
    """n points in `centres` unit-variance blobs whose centres are `spread` apart along random directions"""
    rng = np.random.default_rng(1000 + 17 * dim + seed)
    c = rng.standard_normal((centres, dim))
    c = c / np.linalg.norm(c, axis=1, keepdims=True) * spread * np.arange(centres)[:, None]
    which = rng.integers(0, centres, n)
    return np.ascontiguousarray(c[which] + rng.standard_normal((n, dim)) + 3.0, F32), which


def blob_fixture(dim):
    """-> (points, radius_sq): 1500 points in four blobs, the radius at the 85 % quantile of the nearest-neighbour distances"""
    def make():
        p, _ = blobs(dim)
        return p, radius_for(p, 0.85)
    return _once(("blobs", dim), make)


SIZE_DIMS = (2, 5, 6, 16)
SIZES = (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 4097)


def size_fixture(n, dim):
    def make():
        p, _ = blobs(dim, n=n, seed=n, centres=3)
        return p, (radius_for(p, 0.8) if n > 2 else F32(1.0e6 if n == 2 else 1.0))      # (two points: joined)
    return _once(("size", n, dim), make)


CHAIN_N, CHAIN_DIM, CHAIN_R2 = 3 * TILE + 5, 5, F32(0.32)


def chain_fixture(gap_at=None, shuffled=False):
    """CHAIN_N points on the diagonal of a 5-D space, 0.25 apart on every axis: consecutive points have d2 = 5 / 16 = 0.3125 exactly, just
    under the radius (0.32), the next ones 1.25.  gap_at: the points after that position sit one more step away (d2 = 1.25 across the gap).
    shuffled: a seeded permutation of the input order -> (points, position of every point along the chain)"""
    def make():
        x = np.arange(CHAIN_N, dtype=np.float64) * 0.25
        if gap_at is not None:
            x[gap_at + 1:] += 0.25
        pos = np.random.default_rng(5).permutation(CHAIN_N) if shuffled else np.arange(CHAIN_N)
        return np.ascontiguousarray(np.repeat(x[pos][:, None], CHAIN_DIM, axis=1), F32), pos
    return _once(("chain", gap_at, shuffled), make)


def lattice_fixture():
    """about half of the 6^4 integer lattice points of 4-D, seeded; radius_sq = 2 exactly: the d2 = 1 shell is joined, the d2 = 2 shell sits
    ON the threshold and is not (strict <)"""
    def make():
        g = np.stack(np.meshgrid(*[np.arange(6)] * 4, indexing="ij"), axis=-1).reshape(-1, 4)
        rng = np.random.default_rng(21)
        keep = rng.random(len(g)) < 0.5
        return np.ascontiguousarray(rng.permutation(g[keep]), F32), F32(2.0)
    return _once("lattice", make)


def duplicates_fixture(dim=6):
    """a sparse cloud (most points singletons at this radius) with 40 rows doubled and 20 tripled: a duplicate is always a neighbour"""
    def make():
        p, _ = blobs(dim, n=600, seed=3)
        r2 = radius_for(p, 0.3)
        rng = np.random.default_rng(8)
        twice, thrice = rng.choice(600, 40, replace=False), rng.choice(600, 20, replace=False)
        q = np.concatenate([p, p[twice], p[thrice], p[thrice]])
        return np.ascontiguousarray(q[rng.permutation(len(q))], F32), r2
    return _once(("dups", dim), make)


def nonfinite_fixture(dim=6):
    """the blob cloud of `dim` dimensions (700 points) with NaN, +inf, -inf and +-1e20 rows written over some of its rows, on different axes
    -> (points, radius_sq, the rows written over)"""
    def make():
        p, _ = blobs(dim, n=700, seed=4)
        r2 = radius_for(p, 0.85)
        p = p.copy()
        rows = np.array([0, 3, 255, 256, 257, 400, 511, 512, 650, 699])
        vals = [np.nan, np.inf, -np.inf, 1e20, -1e20, np.nan, 2e20, np.inf, -3e20, np.nan]
        for k, (r, v) in enumerate(zip(rows, vals)):
            p[r, k % dim] = v
        p[400, :] = np.nan      # a row that is NaN on every axis
        return p, r2, rows
    return _once(("nonfinite", dim), make)


def evaluator_fixture(dim):
    """-> (points, radius_sq, normals, sign-flipped normals, colours): 1200 points in three blobs; every blob's unit normals scatter around a
    direction of its own; rows 10 and 11 are one point twice with one over-long normal (dot = 1.0002 > 1: never similar)"""
    def make():
        p, which = blobs(dim, n=1200, seed=9, centres=3, spread=3.0)
        p = p.copy()
        p[11] = p[10]
        rng = np.random.default_rng(33 + dim)
        axes = rng.standard_normal((3, dim))
        nrm = axes[which] + 0.25 * rng.standard_normal((1200, dim))
        nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F32)
        nrm[10] = 0.0; nrm[10, 0] = 1.0001
        nrm[11] = nrm[10]
        sign = np.where(rng.random(1200) < 0.5, F32(-1.0), F32(1.0))[:, None]
        flipped = (nrm * sign).astype(F32)
        flipped[10] = flipped[11] = nrm[10]
        col = rng.random((1200, 3), dtype=F32)
        return p, radius_for(p, 0.9), nrm, flipped, col
    return _once(("eval", dim), make)


def evaluator_cases(dim):
    """the eight evaluator classes as (name, constructor arguments, Clauses) over evaluator_fixture(dim), each class that has an angle with a
    positive threshold on the normals and a negative one on the sign-flipped normals"""
    p, r2, nrm, flipped, col = evaluator_fixture(dim)
    D, CT = F32(0.6) * r2, F32(0.55)
    out = [("AlwaysTrueEvaluator", (), Clauses()), ("PointsProximityEvaluator", (D,), Clauses(max_distance=D)),
           ("ColorsProximityEvaluator", (col, CT), Clauses(colors=col, color_thresh=CT)),
           ("PointsColorsProximityEvaluator", (col, D, CT), Clauses(colors=col, max_distance=D, color_thresh=CT))]
    for a, nn in ((R3.deg(20.0), nrm), (-R3.deg(20.0), flipped)):
        out += [("NormalsProximityEvaluator", (nn, a), Clauses(normals=nn, max_angle=a, angle_inclusive=True)),
                ("PointsNormalsProximityEvaluator", (nn, D, a), Clauses(normals=nn, max_distance=D, max_angle=a)),
                ("NormalsColorsProximityEvaluator", (nn, col, a, CT), Clauses(normals=nn, colors=col, max_angle=a, color_thresh=CT)),
                ("PointsNormalsColorsProximityEvaluator", (nn, col, D, a, CT), Clauses(normals=nn, colors=col, max_distance=D, max_angle=a, color_thresh=CT))]
    return out


def two_far_blobs(dim=6, axis=4):
    """two unit blobs of 600 points each, 1000 apart along `axis` (far more than the radius) -> (points, radius_sq, axis)"""
    def make():
        p, _ = blobs(dim, n=1200, seed=12, centres=1)
        p = p.copy()
        p[::2, axis] += F32(1000.0)
        return p, radius_for(p, 0.85), axis
    return _once(("far", dim, axis), make)
