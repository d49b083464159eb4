"""Pins tests/_model_refs.py (the integer references the GPU model-kernel tests compare against) on the CPU: against exact
rational arithmetic and against the oracle's KMeans, on small versions of the clouds the GPU tests use."""
from fractions import Fraction

import numpy as np
import pytest

import _model_refs as mr


def _round_f32(fr):
    """the f32 nearest to a Fraction, ties to even (no double rounding through f64)"""
    c = np.float32(float(fr))
    cands = {float(c), float(np.nextafter(c, np.float32(np.inf))), float(np.nextafter(c, np.float32(-np.inf)))}
    best = None
    for v in cands:
        if not np.isfinite(v):
            continue
        err = abs(Fraction(v) - fr)
        even = (int(np.float32(v).view(np.uint32)) & 1) == 0
        key = (err, 0 if even else 1)
        if best is None or key < best[0]:
            best = (key, v)
    return np.float32(best[1])


def _clouds():
    rng = np.random.default_rng(7)
    unit = rng.random((100_003, 3), dtype=np.float32)
    f = lambda a, s=1.0, o=0.0: np.ascontiguousarray((a.astype(np.float64) * s + np.broadcast_to(np.asarray(o, np.float64), (3,))).astype(np.float32))
    return (("unit cube", unit, 64), ("unit cube at 4096", f(unit, 1.0, 4096.0), 64),
            ("extent 1e3 across zero", f(unit[:60_001], 1e3, -500.0), 257),
            ("unit cube at (1e3, -250, 37)", f(unit, 1.0, (1e3, -250.0, 37.0)), 1024),
            ("2^-24 scale", f(unit[:30_001], 2.0 ** -24), 64))


@pytest.mark.parametrize("which", range(5))
def test_integer_sums_give_the_correctly_rounded_mean(orc, which):
    name, x, k = _clouds()[which]
    c0 = x[:: len(x) // k][:k].copy()
    lab, _ = orc.kmeans_assign(x, c0)
    S = mr.scale_for(x)
    sums = mr.kmeans_sums(x, lab, k, S)
    assert sums[:, 3].sum() == len(x) and np.array_equal(sums[:, 3], np.bincount(lab, minlength=k))
    # the integers themselves, against Python's exact integers (every f32 is an integer multiple of 2^-149)
    xi = [[int(v) for v in row] for row in (x.astype(np.float64) * 2.0 ** 149).tolist()]
    tot = [[0, 0, 0] for _ in range(k)]
    for row, j in zip(xi, lab.tolist()):
        t = tot[j]
        t[0] += row[0]; t[1] += row[1]; t[2] += row[2]
    cent = mr.centroids_from_sums(sums, S)
    for j in range(k):
        n_j = int(sums[j, 3])
        assert n_j > 0, (name, j)
        for d in range(3):
            want = _round_f32(Fraction(tot[j][d], n_j << 149))
            assert cent[j, d].view(np.uint32) == want.view(np.uint32), (name, j, d, cent[j, d], want)
    co, lo, it = orc.kmeans(x, c0, max_iter=1, tol=0.0, mode=1)
    assert it == 1 and np.array_equal(lo, lab)
    assert np.array_equal(cent.view(np.uint32), co.view(np.uint32)), (name, int(np.count_nonzero(cent != co)))


def test_fixed_point_rounds_half_to_even_and_keeps_the_sign():
    x = np.array([[0.5, 1.5, 2.5], [-0.5, -1.5, -2.5], [0.75, -0.75, 3.0]], np.float32)
    assert mr.fixed_point(x, 0).tolist() == [[0, 2, 2], [0, -2, -2], [1, -1, 3]]
    assert mr.fixed_point(x, 2).tolist() == [[2, 6, 10], [-2, -6, -10], [3, -3, 12]]
    assert mr.fixed_point(np.float32([2.0 ** 44, -3 * 2.0 ** 44]), -44).tolist() == [1, -3]
    assert mr.fixed_point(np.float32([2.0 ** -30]), 70).tolist() == [1 << 40]
    s = mr.kmeans_sums(x, np.array([1, 1, 0]), 3, 2)
    assert s.tolist() == [[3, -3, 12, 1], [0, 0, 0, 2], [0, 0, 0, 0]]
    assert mr.fixed_point(np.float32([np.nan, np.inf, -np.inf, 1.0]), 3).tolist() == [0, 0, 0, 8]


def test_farthest_key_and_the_empty_cluster_repair_follow_the_oracle(orc):
    rng = np.random.default_rng(11)
    x = rng.random((20_001, 3), dtype=np.float32)
    x[100:200] = x[0:100]      # duplicated points: equal distances, the lowest index is kept
    lab = (np.arange(len(x)) % 3).astype(np.int64)
    c = np.float32([0.5, 0.5, 0.5])
    key = mr.farthest_key(x, lab, 1, c, index_offset=1000)
    m = np.nonzero(lab == 1)[0]
    d = ((c - x[m]) ** 2)
    dist = d[:, 0] + (d[:, 1] + d[:, 2])
    first = m[np.nonzero(dist == dist.max())[0][0]]
    assert key >> 32 == int(dist.max().view(np.uint32)) and 0xFFFFFFFF - (key & 0xFFFFFFFF) == first + 1000
    assert mr.farthest_key(x, lab, 5, c) == 0
    # a far-away initial centroid attracts nothing: one oracle iteration repairs it; the helper restates it on the integers
    c0 = x[:8].copy(); c0[5] = [50.0, 50.0, 50.0]
    S = mr.scale_for(x)
    cent = c0
    for it in range(3):
        lab, _ = orc.kmeans_assign(x, cent)
        new, lab2, _ = mr.lloyd_step(x, lab, cent, S)
        co, lo, _ = orc.kmeans(x, cent, max_iter=1, tol=0.0, mode=1)
        assert np.array_equal(lab2, lo), it
        assert np.array_equal(new.view(np.uint32), co.view(np.uint32)), it
        if it == 0:
            assert np.count_nonzero(lab == 5) == 0 and np.count_nonzero(lab2 == 5) == 1
        cent = co


def test_non_finite_points_mark_their_cluster_only(orc):
    rng = np.random.default_rng(13)
    x = rng.random((20_001, 3), dtype=np.float32)
    x[17] = [np.nan, 0.1, 0.2]
    x[4711] = [0.3, np.inf, 0.9]
    c0 = x[100:108].copy()
    lab, _ = orc.kmeans_assign(x, c0)
    assert lab[17] == 0 and lab[4711] == 0
    S = mr.scale_for(x)
    assert S == 62 - 15 - 0      # (the non-finite points do not set the scale: 20 001 points, finite |x| < 1)
    new, lab2, hs = mr.lloyd_step(x, lab, c0, S)
    co, lo, _ = orc.kmeans(x, c0, max_iter=1, tol=0.0, mode=1)
    assert np.array_equal(np.isnan(new), np.isnan(co)) and np.isnan(new[0, 0]) and np.isinf(new[0, 1]) and np.isfinite(new[0, 2])
    assert np.array_equal(new.view(np.uint32)[~np.isnan(co)], co.view(np.uint32)[~np.isnan(co)])
    fl = mr.kmeans_nonfinite_flags(x, lab, 8)
    assert fl.tolist() == [mr.NF_NAN | (mr.NF_PINF << 3), 0, 0, 0, 0, 0, 0, 0]
