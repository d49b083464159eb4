"""Inputs large enough to drive a capped grid-stride kernel through a second trip, each with its expected result in closed form: O(n) numpy in
f64 from exactly representable inputs (the yardsticks the suite trusts are a Python loop, ns x n or quadratic and cannot serve at these
sizes).  Nothing here runs on a device or calls the library.  tests/test_trip_refs_cpu.py pins every builder, at a small size, against those
yardsticks; tests/test_gpu_grid_trips.py uses them at full size.

    clustered(n, k, dim)          n points in k tight clusters on a coarse lattice, point i in cluster i % k -> mean-shift grouping and shift
    clustered_forms(c, ...)       what mean shift gives on them: every point a seed, seeds of their own, some rows non-finite
    two_sinks(c) / sink_forms     8 data points in two tight clusters that swallow the seeds of clustered(..) between them (N-d shift)
    spread(n, dim)                n distinct points of a unit lattice (tolerance 0: every seed its own cluster)
    chain_nd(n, dim, axis, gaps)  a shuffled chain with gaps along one axis of a dim-dimensional cloud -> connected components
    hull_late(dim)                a cloud whose hull, largest |coordinate| and non-finite rows all lie behind row 262 144
"""
import functools

import numpy as np

import _cc_refs as R3

F32 = np.float32
STEP = 2.0 ** -12      # the members' offsets inside a cluster
# what one trip of each capped grid covers (tests/test_trip_refs_cpu.py checks that the sources still say so)
PRIM_TRIP = 2048 * 256      # prim_blocks(): 2048 blocks of PRIM_THREADS = MS_THREADS = CCN_THREADS = 256 lanes, one item per lane
WAVE_TRIP = 4096 * 4      # k_ms_claim, k_ms_modes: 4096 blocks of MS_WAVES = 4 waves, one leader / cluster per wave
FIRST_TRIP_HULL = 1024 * 256      # k_hull_seed: 1024 blocks of HT = 256 lanes
PCA_TRIP = 2048 * 256      # k_pca_project, k_pca_reconstruct: sp_grid(m, 2048) blocks of SP_THREADS = 256 lanes, one row per lane


def exact_f32(x):
    """x (f64) as f32, after asserting that every entry survives f64 -> f32 -> f64"""
    y = np.ascontiguousarray(x, F32)
    assert np.array_equal(y.astype(np.float64), np.asarray(x, np.float64))
    return y


def lists(labels, k):
    """-> (offsets[k + 1], members[n]): the indices sorted stably by label and where each label's run starts"""
    labels = np.asarray(labels, np.int64)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(labels, minlength=k))]).astype(np.int64)
    return offsets, np.argsort(labels, kind="stable").astype(np.int64)


def means_of(points, labels, k):
    """per label float32(S / W): S the f64 sum of the label's rows (np.add.at), W their number.  On clustered() S is exact: multiples of 2^-12
    below 2^31, in any order.  A label without a row gets NaN."""
    p = np.asarray(points, np.float64)
    S = np.zeros((k, p.shape[1]))
    np.add.at(S, labels, p)
    W = np.bincount(labels, minlength=k).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (S / W[:, None]).astype(F32)


# ---- mean shift ---------------------------------------------------------------------------------------------------------------------
def clustered(n, k, dim=3, spacing=1.0, side=32, radius=0.25, tol=2.0 ** -3):
    """n points in k clusters, point i in cluster i % k.  Cluster c's first member (index c) sits on a lattice of step `spacing`: site
    (c % side, (c // side) % side, c // side^2) in 3-D, (c % side, c // side) on the first two axes otherwise.  Member m = i // k is offset by
    (m % 16, (m // 16) % 16, m // 256) * 2^-12 on the first three axes (two axes: (m % 16, m // 16)); an axis a >= 3 holds the constant
    (a - 2) / 4.  A cluster's diameter stays below a quarter of the grouping tolerance and of the kernel radius, and two clusters are more
    than spacing - diameter > 2 max(radius, tol) apart: a ball around any point of a cluster, or around its mean, holds that cluster alone.
    -> dict(points, n, k, dim, radius, tol, labels, leaders, offsets, members, means, modes): the grouping of the points as seeds (labels
    i % k, leaders 0 .. k - 1, lists stable by label), the per-cluster mean float32(S / W) -- where every seed of the cluster goes in one shift
    -- and the modes, which are those means: before the shift as the exact f64 sum of the members over their number, after it as the f64 sum
    of W copies of one f32 number (24 + 11 bits: exact) over W."""
    assert 2 <= dim <= 16 and 1 <= k <= n
    i = np.arange(n)
    c, m = i % k, i // k
    p = np.zeros((n, dim))
    if dim == 3:
        site = np.stack([c % side, (c // side) % side, c // (side * side)], axis=1)
    else:
        site = np.stack([c % side, c // side], axis=1)
    p[:, :site.shape[1]] = site * float(spacing)
    off = np.stack([m % 16, (m // 16) % 16, m // 256], axis=1) if dim >= 3 else np.stack([m % 16, m // 16], axis=1)
    p[:, :off.shape[1]] += off * STEP
    for a in range(3, dim):
        p[:, a] = (a - 2) / 4.0
    diameter = float(np.linalg.norm(off.max(axis=0) * STEP))
    assert diameter < min(tol, radius) / 4 and spacing - diameter > 2 * max(radius, tol)
    points = exact_f32(p)
    labels = c.astype(np.int64)
    offsets, members = lists(labels, k)
    means = means_of(points, labels, k)
    assert np.abs(p).max() * n / k < 2.0 ** 31 * STEP      # S is exact
    return {"points": points, "n": n, "k": k, "dim": dim, "side": side, "spacing": float(spacing), "radius": radius, "tol": tol, "labels": labels, "leaders": np.arange(k, dtype=np.int64),
            "offsets": offsets, "members": members, "means": means, "modes": means}


def clustered_forms(c, max_iter, bad_rows=None, reverse_seeds=False):
    """What mean shift with c's radius and tolerance gives on c["points"] -> dict(points, seeds, shifted, labels, offsets, members, modes,
    iterations, passes).
      bad_rows       {row: (axis, value)}: those rows of the points get a non-finite entry (every point is a seed: the rows become NaN
                     singletons, numbered after the k clusters in ascending index -- every bad row lies above k --, `iterations` is max_iter, and
                     every other seed goes to the mean of its cluster without those rows)
      reverse_seeds  the seeds are an array of their own, the points in reverse order (seed j is point n - 1 - j; j -> (n - 1 - j) % k has
                     period k, so the first k seeds lead k different clusters and seed j is in cluster j % k)
    max_iter = 0: the seeds as they came, grouped.  Otherwise the first pass takes every finite seed to its cluster's mean and the second pass
    finds it converged (it does not move: d2 = 0)."""
    n, k, pts = c["n"], c["k"], c["points"]
    bad = np.zeros(n, bool)
    if bad_rows:
        assert not reverse_seeds and min(bad_rows) >= k and max_iter > 0
        pts = pts.copy()
        for row, (axis, value) in bad_rows.items():
            pts[row, axis] = value
            bad[row] = True
        assert np.array_equal(bad, ~np.isfinite(pts).all(axis=1))
    cluster = c["labels"]
    means = means_of(pts[~bad], cluster[~bad], k) if bad.any() else c["means"]
    assert np.isfinite(means).all()
    if reverse_seeds:
        seeds = np.ascontiguousarray(pts[::-1])
        lead_cluster = (n - 1 - np.arange(k)) % k      # the cluster seed j < k leads
        assert len(set(lead_cluster.tolist())) == k
        rank_of = np.empty(k, np.int64)
        rank_of[lead_cluster] = np.arange(k)
        labels = rank_of[cluster[::-1]]
        assert np.array_equal(labels, np.arange(n) % k)
        modes = means[lead_cluster]
    else:
        seeds, labels, modes = pts, cluster.copy(), means
    shifted = seeds.copy() if max_iter == 0 else means[(cluster[::-1] if reverse_seeds else cluster)]
    n_clusters = k
    if bad.any():
        shifted = shifted.copy()
        shifted[bad] = np.nan
        labels[bad] = k + np.arange(int(bad.sum()))
        n_clusters = k + int(bad.sum())
        modes = np.concatenate([modes, np.full((int(bad.sum()), c["dim"]), np.nan, F32)])
    offsets, members = lists(labels, n_clusters)
    if max_iter == 0:
        modes = means_of(seeds, labels, n_clusters)
    return {"points": pts, "seeds": seeds if reverse_seeds else None, "shifted": shifted, "labels": labels, "offsets": offsets, "members": members, "modes": modes,
            "iterations": 0 if max_iter == 0 else (max_iter if bad.any() else 2), "passes": 0 if max_iter == 0 else 2}


SINK_RADIUS = 79.75      # its square, 6360.0625, is an f32 number


def two_sinks(c):
    """8 data points in two tight clusters, A around (-64, 0) and B around (side - 1 + 64, y_max), for the seeds c = clustered(n, k, dim, side=32)
    whose sites fill x = 0 .. 31, y = 0 .. y_max <= 9: with SINK_RADIUS a seed whose site has x <= 15 holds all of A and nothing of B in its
    ball, one with x >= 16 all of B and nothing of A (asserted here for every seed, in f64, with a margin no f32 rounding of d2 reaches).
    On the other axes the data points sit where the seeds do.  -> (points[8, dim], in_a[n])"""
    assert c["dim"] != 3 and c["side"] == 32 and c["spacing"] == 1.0 and c["k"] >= 32
    dim, y_max = c["dim"], (c["k"] - 1) // 32
    assert y_max <= 9
    p = np.zeros((8, dim))
    for a in range(3, dim):
        p[:, a] = (a - 2) / 4.0
    corner = np.array([[0, 0], [1, 0], [0, 1], [1, 1]]) * 0.125
    p[:4, :2] = np.array([-64.0, 0.0]) + corner
    p[4:, :2] = np.array([31.0 + 64.0, float(y_max)]) + corner
    points = exact_f32(p)
    s = c["points"].astype(np.float64)
    in_a = (c["labels"] % 32) <= 15
    r2 = SINK_RADIUS * SINK_RADIUS
    for j in range(8):
        d2 = ((s - p[j]) ** 2).sum(axis=1)
        inside = in_a if j < 4 else ~in_a
        assert (d2[inside] < r2 - 1.0).all() and (d2[~inside] > r2 + 1.0).all()
    return points, in_a


def sink_forms(c, data, in_a, max_iter=3):
    """mean shift of c's points as seeds over the 8 data points of two_sinks: one pass takes a seed to the mean of A or of B (an exact f64 sum of
    four numbers over 4), the second finds it converged, and the grouping leaves two clusters led by seeds 0 (A) and 16 (B)"""
    mean = np.stack([data[:4].astype(np.float64).sum(axis=0) / 4.0, data[4:].astype(np.float64).sum(axis=0) / 4.0]).astype(F32)
    # the second pass: a seed at A's mean holds A alone (B is 159 away), and the other way round
    assert np.linalg.norm(mean[0].astype(np.float64) - mean[1].astype(np.float64)) > 2 * SINK_RADIUS - 1
    labels = np.where(in_a, 0, 1).astype(np.int64)
    assert labels[0] == 0 and labels[16] == 1 and (labels[:16] == 0).all()
    offsets, members = lists(labels, 2)
    return {"shifted": mean[labels], "labels": labels, "offsets": offsets, "members": members, "modes": mean, "iterations": 2, "passes": 2, "leaders": np.array([0, 16])}


def spread(n, dim):
    """n distinct points of the unit lattice: the digits of the index in the smallest base whose dim-th power holds n (two indices below
    base^dim differ in a digit)"""
    base = 1
    while base ** dim < n:
        base += 1
    i = np.arange(n)
    return exact_f32(np.stack([(i // base ** a) % base for a in range(dim)], axis=1).astype(np.float64))


# ---- connected components -----------------------------------------------------------------------------------------------------------
def chain_nd(n, dim, axis, gaps, seed=5):
    """The shuffled chain of test_gpu_components.py (spacing 0.75 under radius 1, the k-th gap 0.5 + 0.25 k wider: 1.25, 1.5, ... between
    neighbours), laid on `axis` of a dim-dimensional cloud whose other coordinates are the constants 0.5, 1, 1.5, ...: a pair's d2 is the exact
    square of its distance along the axis, whatever the order of the sum.  -> (points, (labels, offsets, members), segment sizes in chain
    order): the roots by _cc_refs.chain_roots' rule on that axis, finished by _cc_refs.finish."""
    x = np.arange(n, dtype=np.float64) * 0.75
    for k, at in enumerate(gaps):
        x[at + 1:] += 0.5 + 0.25 * k
    pos = np.random.default_rng(seed).permutation(n)
    p = np.repeat(0.5 * (1.0 + np.arange(dim))[None, :], n, axis=0)
    p[:, axis] = x[pos]
    points = exact_f32(p)
    line = np.zeros((n, 3), F32)
    line[:, 0] = points[:, axis]
    root = R3.chain_roots(line, F32(1.0))
    edges = [-1] + list(gaps) + [n - 1]
    return points, R3.finish(n, root), [edges[j + 1] - edges[j] for j in range(len(edges) - 1)]


# ---- convex hull --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hull_late(dim, shell=200, seed=11):
    """262 144 rows inside the ball of radius 0.25 (k_hull_seed's first trip), then `shell` rows on the unit sphere (circle), the 2 dim axis
    points +-e_a first; then five rows with NaN or infinite entries; then copies of three shell rows.  The shell row that is the extreme of the
    diagonal direction (+, +, +), by the kernel's own f32 sum, is copied to row 7 as well: that extreme ties across the two trips, and of exact
    duplicates the lowest index is the vertex.  Every hull vertex but row 7, the largest |coordinate| (1, on the axis points; row 7 stays
    below it) and every non-finite row lie behind the first trip.  -> (points, dict(first_late, shell, tie_source, copies, copy_sources): row numbers)"""
    assert dim in (2, 3)
    rng = np.random.default_rng(seed + dim)
    g = rng.standard_normal((FIRST_TRIP_HULL, dim))
    inner = g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0, 0.249, (FIRST_TRIP_HULL, 1))
    g = rng.standard_normal((shell - 2 * dim, dim))
    sh = np.concatenate([np.eye(dim), -np.eye(dim), g / np.linalg.norm(g, axis=1, keepdims=True)]).astype(F32)
    assert (np.abs(sh[2 * dim:]) < 1).all()      # the axis points alone reach 1
    diag = (sh[:, 0] + sh[:, 1]) + sh[:, 2] if dim == 3 else sh[:, 0] + sh[:, 1]
    assert diag.dtype == F32
    tie = int(np.argmax(diag))
    assert (diag == diag[tie]).sum() == 1 and tie >= 2 * dim
    bad = np.array([[np.nan, 0, 0], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [0.2, 0.2, np.nan], [np.inf, np.inf, np.inf]] if dim == 3 else
                   [[np.nan, 0], [np.inf, 0.5], [0.5, -np.inf], [0.2, np.nan], [np.inf, np.inf]])
    copies = [tie, 0, 2 * dim + 3]
    pts = np.concatenate([inner.astype(F32), sh, bad.astype(F32), sh[copies]])
    pts[7] = sh[tie]
    pts = np.ascontiguousarray(pts, F32)
    assert (np.linalg.norm(pts[:FIRST_TRIP_HULL].astype(np.float64), axis=1)[np.arange(FIRST_TRIP_HULL) != 7] < 0.25).all()
    pts.setflags(write=False)
    return pts, {"first_late": FIRST_TRIP_HULL, "shell": shell, "tie_source": FIRST_TRIP_HULL + tie, "copies": [FIRST_TRIP_HULL + shell + 5 + j for j in range(3)],
                 "copy_sources": [FIRST_TRIP_HULL + j for j in copies]}
