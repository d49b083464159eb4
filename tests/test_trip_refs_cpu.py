"""CPU: the builders of tests/_trip_refs.py and their closed forms, each at a small size against the yardstick the suite already trusts
(_meanshift_refs, _meanshift_nd_refs, _ccn_refs, _hull_refs), and the caps those builders are sized for against the sources."""
import os
import re

import numpy as np
import pytest

import _ccn_refs as RC
import _hull_refs as RH
import _meanshift_nd_refs as RN
import _meanshift_refs as R3
import _trip_refs as T

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cilantro_amd", "csrc")
EXACT = ("labels", "offsets", "members")


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_caps_are_the_sources():
    prims = src("device_prims.hpp")
    assert "constexpr int PRIM_THREADS = 256;" in prims and "std::min<size_t>((n + PRIM_THREADS - 1) / PRIM_THREADS, 2048)" in prims
    shared = src("mean_shift_device.hpp")
    assert "constexpr int MS_THREADS = 256;" in shared and "MS_WAVES = MS_THREADS / 64" in shared and "ms_launch(n_clusters, MS_WAVES), 4096u)" in shared
    assert "ms_launch(n_u, MS_WAVES), 4096u)" in src("mean_shift.hip")
    assert T.PRIM_TRIP == 2048 * 256 and T.WAVE_TRIP == 4096 * (256 // 64)
    hull = src("convex_hull.hip")
    assert "constexpr int HT = 256;" in hull and re.search(r"k_hull_seed<DIM>, dim3\(std::min<uint32_t>\(nblocks_all, 1024u\)\), dim3\(HT\)", hull)
    assert T.FIRST_TRIP_HULL == 1024 * 256
    pca = src("pca.hip")
    assert "constexpr int SP_THREADS = 256;" in src("subspace_device.hpp") and pca.count("dim3(sp_grid(m, 2048)), dim3(SP_THREADS)") == 2
    assert T.PCA_TRIP == 2048 * 256
    assert "constexpr int CC_THREADS = 256;" in src("components_device.hpp") and "CCN_THREADS == CC_THREADS" in src("components_nd.hip")


def same(got, want, what=EXACT + ("shifted", "modes")):
    for k in what:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        if k in ("shifted", "modes"):
            assert got[k].dtype == want[k].dtype == np.float32 and got[k].tobytes() == np.asarray(want[k]).tobytes(), k      # bit for bit


@pytest.mark.parametrize("n,k", [(700, 37), (1000, 3)])
def test_clustered_3d_is_what_the_mean_shift_yardsticks_give(n, k):
    c = T.clustered(n, k)
    prm = dict(kernel_radius=c["radius"], cluster_tol=c["tol"])
    labels, leaders = R3.first_fit(c["points"], c["tol"])
    assert np.array_equal(labels, c["labels"]) and np.array_equal(leaders, c["leaders"])
    # grouping alone, then shift and group: every point a seed
    for max_iter in (0, 3):
        want = T.clustered_forms(c, max_iter)
        got = R3.contract(c["points"], None, max_iter=max_iter, **prm)
        same(got, want)
        assert got["iterations"] == want["iterations"] == (2 if max_iter else 0) and np.array_equal(got["leaders"], c["leaders"])
        assert np.array_equal(want["modes"], c["modes"]) and np.array_equal(want["labels"], c["labels"])
    assert np.array_equal(got["shifted"], c["means"][c["labels"]])
    # the seeds as an array of their own
    want = T.clustered_forms(c, 3, reverse_seeds=True)
    got = R3.contract(c["points"], want["seeds"], max_iter=3, **prm)
    same(got, want)
    assert got["iterations"] == 2 and np.array_equal(got["leaders"], np.arange(k))
    # some rows non-finite: NaN singletons behind the k clusters, the others see their cluster without those rows
    bad = {n - 50: (0, np.nan), n - 49: (1, np.inf), n - 3: (2, -np.inf), n - 1: (1, np.nan)}
    want = T.clustered_forms(c, 3, bad_rows=bad)
    got = R3.contract(want["points"], None, max_iter=3, **prm)
    same(got, want)
    assert got["iterations"] == want["iterations"] == 3 and len(got["leaders"]) == k + 4 and np.isnan(got["shifted"][list(bad)]).all()
    touched = sorted({r % k for r in bad})
    assert not np.array_equal(want["modes"][touched], c["modes"][touched])      # the closed form without the rows is another one


@pytest.mark.parametrize("dim", [2, 16])
@pytest.mark.parametrize("n,k", [(700, 37), (1000, 3)])
def test_clustered_nd_is_what_the_nd_yardsticks_give(n, k, dim):
    c = T.clustered(n, k, dim)
    assert c["points"].shape == (n, dim)
    labels, leaders = RN.first_fit(c["points"], c["tol"])
    assert np.array_equal(labels, c["labels"]) and np.array_equal(leaders, c["leaders"])
    for max_iter in (0, 3):
        want = T.clustered_forms(c, max_iter)
        got = RN.contract_nd(c["points"], None, c["radius"], max_iter, c["tol"])
        same(got, want)
        assert got["iterations"] == want["iterations"] == (2 if max_iter else 0)


@pytest.mark.parametrize("dim", [2, 16])
def test_two_sinks_swallow_the_clustered_seeds(dim):
    c = T.clustered(1300, 300, dim)
    data, in_a = T.two_sinks(c)
    want = T.sink_forms(c, data, in_a)
    got = RN.contract_nd(data, c["points"], T.SINK_RADIUS, 3, c["tol"])
    same(got, want)
    assert got["iterations"] == 2 and np.array_equal(got["leaders"], want["leaders"]) and 0 < in_a.sum() < 1300
    assert np.float32(T.SINK_RADIUS) * np.float32(T.SINK_RADIUS) == T.SINK_RADIUS ** 2      # radius_sq is exact


def test_spread_is_one_cluster_per_seed_at_tolerance_zero():
    for n, dim in ((200, 3), (200, 5)):
        s = T.spread(n, dim)
        assert s.shape == (n, dim) and len(np.unique(s, axis=0)) == n
        labels, leaders = RN.first_fit(s, 0.0)
        assert np.array_equal(labels, np.arange(n)) and np.array_equal(leaders, np.arange(n))
    assert T.spread(T.PRIM_TRIP + 12, 3).max() < 128      # a small box: the seeds' grid stays small


@pytest.mark.parametrize("dim,axis", [(2, 1), (16, 0)])
def test_chain_nd_is_what_the_components_yardstick_gives(dim, axis):
    gaps = (100, 700, 1200, 1990)
    p, want, sizes = T.chain_nd(2001, dim, axis, gaps)
    got = RC.components(p, np.float32(1.0))
    for a, b in zip(got, want):
        assert np.array_equal(a, b)
    assert sizes == [101, 600, 500, 790, 10] and sorted(np.diff(want[1]).tolist()) == sorted(sizes) and RC.pick_axis(p) == axis
    others = np.delete(p, axis, axis=1)
    assert (others == others[0]).all() and (others != 0).all()


@pytest.mark.parametrize("dim", [3, 2])
def test_hull_late_keeps_everything_that_matters_behind_the_first_trip(dim):
    pts, meta = T.hull_late(dim)
    late = meta["first_late"]
    assert late == T.FIRST_TRIP_HULL and pts.shape == (late + meta["shell"] + 5 + 3, dim)
    ref = RH.ref_hull(pts)
    v = ref["vertex_point_indices"].astype(np.int64)
    assert ref["n_nonfinite"] == 5 and not np.isfinite(pts[late + meta["shell"]:late + meta["shell"] + 5]).all(axis=1).any() and np.isfinite(pts[:late]).all()
    assert v[0] == 7 and (v[1:] >= late).all() and len(v) > 50      # no vertex in the first trip but the tied row
    assert meta["tie_source"] not in v and not set(meta["copies"]) & set(v.tolist())      # of exact duplicates the lowest index
    assert set(meta["copy_sources"][1:]) <= set(v.tolist()) and pts[meta["copies"]].tobytes() == pts[meta["copy_sources"]].tobytes()
    assert pts[7].tobytes() == pts[meta["tie_source"]].tobytes()
    # the band: the largest |coordinate| is 1 and lies behind the first trip -- a seed pass that missed the second trip would get another band
    assert RH.tol_of(pts) == 2.0 ** -44 and RH.tol_of(pts[:late]) < RH.tol_of(pts) and ref["tol"] == RH.tol_of(pts)
    assert float(np.abs(pts[late:][np.isfinite(pts[late:]).all(axis=1)]).max()) == 1.0
