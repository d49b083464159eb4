"""Searches on clouds that hold NaN / +-inf points (depth-sensor frames do), on the GPU: a point with a non-finite coordinate keeps its
index, is never returned as a neighbour and finds nothing as a query; every other point and query gets what the same call returns
on the clouds with those rows removed, indices mapped back (include/cilantro_hip/c_api.h, "Non-finite points").

The expectations are the CPU oracle's on the filtered clouds (tests/_nonfinite_refs.py; tests/test_nonfinite_refs_cpu.py holds them
against a brute force over the unfiltered arrays and shows the inputs to be tie-free).  Every comparison is exact: indices and
counts with np.array_equal, distances on their bits.  Tie order on such clouds is not defined, so no order table may be built."""
import subprocess
import sys

import numpy as np
import pytest

import _nonfinite_refs as nf
import _normal_refs as nr
from cilantro_amd import capi

pytestmark = pytest.mark.gpu

FORMS = tuple((("tiled", t), ("group_search", g)) for t in (0, 2) for g in (0, 8))
_cases = {}


def _case(orc, n, dst_rows, src_rows):
    key = (n, dst_rows, src_rows)
    if key not in _cases:
        _cases[key] = nf.pair_case(orc, n, dst_rows, src_rows)
    return _cases[key]


@pytest.fixture(scope="module")
def Context(hip_lib):
    from cilantro_amd.icp import Context as C

    return C


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _context(Context, dst, src, opts=()):
    ctx = Context()
    for k, v in opts:
        ctx.set_option(k, v)
    ctx.set_target(dst)
    ctx.set_source(src)
    return ctx


def _check_forward(Context, orc, c, opts):
    """SECOND_TO_FIRST under the pair's transform: the pair list and the per-source matches against the expectation"""
    di, si, dv, nn, nd2 = nf.expected_nn(orc, c["dst"], c["q"], c["max_sq"])
    ctx = _context(Context, c["dst"], c["src"], opts)
    n = ctx.find_correspondences(c["T"], c["max_sq"])
    g1, g2, gv = ctx.get_correspondences()
    idx, d2 = ctx.get_nn()
    builds = ctx.tie_order_info()["builds"]
    ctx.close()
    assert n == len(di) and np.array_equal(g1, di) and np.array_equal(g2, si) and np.array_equal(_bits(gv), _bits(dv)), opts
    gi = idx.astype(np.int64); gi[idx == capi.NONE_IDX] = -1
    assert np.array_equal(gi, nn), (opts, np.nonzero(gi != nn)[0][:10])
    assert np.array_equal(_bits(d2[nn >= 0]), _bits(nd2[nn >= 0])), opts
    assert (idx[~nf.finite_mask(c["src"])] == capi.NONE_IDX).all()
    assert builds == 0, opts
    return len(di)


# ---- SECOND_TO_FIRST: target spoiled, source spoiled, both -----------------------------------------------------------------------
@pytest.mark.parametrize("rows", nf.ROW_SETS)
@pytest.mark.parametrize("side", ("target", "source", "both"))
def test_forward_search_with_spoiled_rows(Context, orc, side, rows):
    c = _case(orc, 20000, rows if side != "source" else None, rows if side != "target" else None)
    for opts in FORMS:
        assert _check_forward(Context, orc, c, opts) > 15000


@pytest.mark.parametrize("n", (2049, 257))
@pytest.mark.parametrize("side", ("target", "source", "both"))
def test_forward_search_with_spoiled_rows_at_the_edge_sizes(Context, orc, side, n):
    c = _case(orc, n, "mixed" if side != "source" else None, "mixed" if side != "target" else None)
    for opts in FORMS:
        assert _check_forward(Context, orc, c, opts) > n // 2


# ---- FIRST_TO_SECOND / BOTH: the grid over the (transformed) source ----------------------------------------------------------------
@pytest.mark.parametrize("n", nf.PAIR_SIZES)
@pytest.mark.parametrize("direction,reciprocal", [(1, False), (2, False), (2, True)])
def test_search_directions_with_both_clouds_spoiled(Context, orc, direction, reciprocal, n):
    c = _case(orc, n, "mixed", "mixed")
    o1, o2, ov = nf.expected_dir(orc, c["dst"], c["q"], c["max_sq"], direction, reciprocal)
    ctx = _context(Context, c["dst"], c["src"], (("search_direction", direction), ("require_reciprocality", 1 if reciprocal else 0)))
    ctx.find_correspondences(c["T"], c["max_sq"], count=False)
    g1, g2, gv = ctx.get_correspondences()
    builds = ctx.tie_order_info()["builds"]
    ctx.close()
    assert len(o1) > n // 2 and len(g1) == len(o1)
    assert np.array_equal(g1, o1) and np.array_equal(g2, o2) and np.array_equal(_bits(gv), _bits(ov))
    assert builds == 0


# ---- transforms that are not numbers ---------------------------------------------------------------------------------------------
_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import _nonfinite_refs as nf
from oracle import oracle as orc
from cilantro_amd.icp import Context
from cilantro_amd.normal_estimation import KDTree3f
what = sys.argv[2]
if what == "transforms":
    c = nf.pair_case(orc, 20000)
    Tn = c["T"].copy(); Tn[1, 2] = np.nan
    Ti = c["T"].copy(); Ti[0, 3] = np.inf
    for T in (Tn, Ti):
        for direction in (0, 1, 2):
            for opts in ((("tiled", 0),), (("tiled", 2),)):
                ctx = Context()
                for k, v in opts + (("search_direction", direction),):
                    ctx.set_option(k, v)
                ctx.set_target(c["dst"]); ctx.set_source(c["src"])
                assert ctx.find_correspondences(T, c["max_sq"]) == 0        # (raises unless the call returned CILHIP_OK)
                assert len(ctx.get_correspondences()[0]) == 0
                ctx.close()
else:
    for n in (5, 257):
        bad = nf.spoil(np.zeros((n, 3), np.float32), np.arange(n), nf.KINDS)
        good = nf.pair_case(orc, 257)["dst"]
        for dst, src in ((bad, good), (good, bad), (bad, bad)):
            for direction in (0, 1, 2):
                for opts in ((("tiled", 0), ("group_search", 0)), (("tiled", 2),), (("tiled", 0), ("group_search", 8))):
                    ctx = Context()
                    for k, v in opts + (("search_direction", direction),):
                        ctx.set_option(k, v)
                    ctx.set_target(dst); ctx.set_source(src)
                    assert ctx.find_correspondences(np.eye(4), 3.0e38) == 0
                    assert len(ctx.get_correspondences()[0]) == 0
                    if direction == 0:
                        assert (ctx.get_nn()[0] == 0xFFFFFFFF).all()
                    assert ctx.grid_info().nx >= 5
                    ctx.close()
        tree = KDTree3f(bad)
        for q in (good, None):
            idx, d2, cnt = tree.kNNSearch(q, 3)
            assert (cnt == 0).all() and (idx == -1).all()
            off, ri, rd = tree.radiusSearch(q, 1.0)
            assert (off == 0).all() and len(ri) == 0
        idx, d2, cnt = KDTree3f(good).kNNSearch(bad, 3)
        assert (cnt == 0).all() and (idx == -1).all()
print("CHILD OK")
"""


@pytest.mark.parametrize("what", ("transforms", "all_rows"))
def test_nothing_to_find_returns_nothing_in_time(hip_lib, orc, what):
    """a transform with one NaN entry / an infinite translation, and clouds whose every row is non-finite (n = 5 and 257: as target, as
    source, as k-NN reference): zero correspondences in all three directions and CILHIP_OK.  In a child process with a time limit: these
    are the inputs that used to send the grid's dimension loop round for ever."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _CHILD, root, what], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "CHILD OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- a target with one finite point ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 3, 65))
def test_target_with_one_finite_point(Context, orc, n):
    c = _case(orc, 257, None, "mixed")
    dst = nf.spoil(np.zeros((n, 3), np.float32), np.arange(n), nf.KINDS)
    keep = n // 2
    dst[keep] = [0.5, 0.5, 0.5]
    r2 = np.float32(0.2)
    with np.errstate(invalid="ignore"):
        want = np.where(nf.brute_d2(dst[keep:keep + 1], c["q"])[:, 0] < r2, keep, -1)
    assert 10 < (want >= 0).sum() < len(want)
    for opts in FORMS:
        ctx = _context(Context, dst, c["src"], opts)
        ctx.find_correspondences(c["T"], r2, count=False)
        idx, d2 = ctx.get_nn()
        ctx.close()
        gi = idx.astype(np.int64); gi[idx == capi.NONE_IDX] = -1
        assert np.array_equal(gi, want), opts


# ---- k-NN and radius lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", nf.PAIR_SIZES)
def test_knn_lists_with_a_spoiled_reference(hip_lib, orc, n):
    from cilantro_amd.normal_estimation import KDTree3f

    c = _case(orc, n, "mixed", "mixed")
    tree = KDTree3f(c["dst"])
    r2 = np.float32((2.5 * c["h"]) ** 2)
    for q in (c["q"], None):
        spoiled = ~nf.finite_mask(c["dst"] if q is None else q)
        for k in (1, 8, 32):
            for rad in (np.inf, r2):
                gi, gd, gc = tree.kNNSearch(q, k) if np.isinf(rad) else tree.kNNInRadiusSearch(q, k, rad)
                oi, od, oc = nf.expected_knn(orc, c["dst"], q, k, rad)
                assert np.array_equal(gc, oc), (k, rad)
                assert np.array_equal(gi, oi), (k, rad, np.nonzero((gi != oi).any(axis=1))[0][:5])
                live = oi >= 0
                assert np.array_equal(_bits(gd[live]), _bits(od[live])) and np.isfinite(gd[live]).all(), (k, rad)
                assert (gc[spoiled] == 0).all() and (gi[spoiled] == -1).all()
                if np.isinf(rad):
                    assert (gc[~spoiled] == min(k, int(nf.finite_mask(c["dst"]).sum()))).all()


def test_knn_never_lists_an_infinite_distance(hip_lib, orc):
    """3 finite + 2 infinite + 2 NaN points, k = 5, unbounded: three neighbours, no entry at distance inf"""
    from cilantro_amd.normal_estimation import KDTree3f

    ref = np.float32([[0, 0, 0], [np.inf, 0, 0], [1, 0, 0], [np.nan, 1, 1], [0, 2, 0], [0, -np.inf, 0], [np.nan, np.nan, np.nan]])
    q = np.float32([[0.1, 0.1, 0.1], [5, 5, 5]])
    for qq in (q, None):
        gi, gd, gc = KDTree3f(ref).kNNSearch(qq, 5)
        oi, od, oc = nf.expected_knn(orc, ref, qq, 5)
        fin = nf.finite_mask(ref if qq is None else qq)
        assert (gc[fin] == 3).all() and (gc[~fin] == 0).all() and np.array_equal(gc, oc)
        assert np.array_equal(gi, oi) and np.isfinite(gd[gi >= 0]).all() and np.array_equal(_bits(gd[gi >= 0]), _bits(od[oi >= 0]))


@pytest.mark.parametrize("n", nf.PAIR_SIZES)
def test_radius_lists_with_a_spoiled_reference(hip_lib, orc, n):
    from cilantro_amd.normal_estimation import KDTree3f

    c = _case(orc, n, "mixed", "mixed")
    tree = KDTree3f(c["dst"])
    for q in (c["q"], None):
        spoiled = ~nf.finite_mask(c["dst"] if q is None else q)
        for r2 in (0.0, np.float32(2.0 * c["h"] ** 2), np.float32(9.0 * c["h"] ** 2)):      # squared radii: 0, 2 and 9 grid spacings squared
            off, idx, d2 = tree.radiusSearch(q, r2)
            ooff, oidx, od2 = nf.expected_radius(orc, c["dst"], q, r2)
            assert np.array_equal(off, ooff), r2
            assert np.array_equal(idx, oidx) and np.array_equal(_bits(d2), _bits(od2)), r2
            assert (np.diff(off)[spoiled] == 0).all()
            assert r2 == 0.0 or off[-1] > 0


# ---- normals -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (20000, 257))
def test_normals_with_spoiled_rows(hip_lib, orc, n):
    """NaN rows for the spoiled points; every other row byte for byte the row of the run on the filtered cloud (same lists, same
    arithmetic), which itself lies inside the f64 bound of tests/_normal_refs.py"""
    from cilantro_amd.normal_estimation import NormalEstimation3f

    c = _case(orc, n, "mixed", None)
    x = c["dst"]
    fin = nf.finite_mask(x)
    xf = np.ascontiguousarray(x[fin])
    vp = np.float32([0.5, 0.5, 10.0])
    r2 = np.float32(2.25 * c["h"] ** 2)      # 1.5 grid spacings: about 14 points per ball, some with fewer than 3 (NaN rows on both sides)
    for call in (("knn", 10, np.inf), ("knn", 12, r2), ("radius", r2)):
        def run(cloud):
            ne = NormalEstimation3f(cloud).setViewPoint(vp)
            return ne._run(call[1], float(call[2]), True) if call[0] == "knn" else ne._run_radius(float(call[1]), True)
        ng, cg = run(x)
        nf_, cf_ = run(xf)
        assert np.isnan(ng[~fin]).all() and np.isnan(cg[~fin]).all(), call
        assert ng[fin].tobytes() == nf_.tobytes() and cg[fin].tobytes() == cf_.tobytes(), call
        idx, cnt, _ = nr.oracle_lists(orc, xf, call)
        res = nr.check(nr.reference(xf, idx, cnt), nf_, cf_, xf, vp)
        assert not nr.violations(res), (call, nr.violations(res))


# ---- finite but hostile ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hostile(orc):
    return nf.hostile_case(orc)


def test_far_outliers_forward_and_directions(Context, orc, hostile):
    """two far outliers collapse the grid to a few huge cells (the tiled path must fall back cleanly): every form against the oracle
    on the full clouds"""
    c = hostile
    tree = orc.KDTree(c["dst"])
    o1, o2, ov = tree.find_correspondences(c["q"], float(c["max_sq"]))
    assert set(o2[-2:]) == {20000, 20001} and set(o1[-2:]) == {20000, 20001}      # the outliers match each other
    for opts in FORMS:
        ctx = _context(Context, c["dst"], c["src"], opts)
        n = ctx.find_correspondences(c["T"], c["max_sq"])
        g1, g2, gv = ctx.get_correspondences()
        gi = ctx.grid_info()
        ctx.close()
        assert n == len(o1) and np.array_equal(g1, o1) and np.array_equal(g2, o2) and np.array_equal(_bits(gv), _bits(ov)), opts
        assert max(gi.nx, gi.ny, gi.nz) <= 2048 and gi.cell > 100.0      # (a few huge cells)
    for direction, reciprocal in ((1, False), (2, False), (2, True)):
        d1, d2_, dv = orc.find_correspondences_dir(c["dst"], c["q"], float(c["max_sq"]), direction, reciprocal)
        ctx = _context(Context, c["dst"], c["src"], (("search_direction", direction), ("require_reciprocality", 1 if reciprocal else 0)))
        ctx.find_correspondences(c["T"], c["max_sq"], count=False)
        g1, g2, gv = ctx.get_correspondences()
        ctx.close()
        assert np.array_equal(g1, d1) and np.array_equal(g2, d2_) and np.array_equal(_bits(gv), _bits(dv)), (direction, reciprocal)


def test_far_outliers_knn_and_radius_lists(hip_lib, orc, hostile):
    from cilantro_amd.normal_estimation import KDTree3f

    c = hostile
    tree_o, tree_g = orc.KDTree(c["dst"]), KDTree3f(c["dst"])
    r2 = np.float32((2.5 * c["h"]) ** 2)
    for k, rad in ((1, np.inf), (8, np.inf), (32, r2), (8, r2)):
        gi, gd, gc = tree_g.kNNSearch(c["q"], k) if np.isinf(rad) else tree_g.kNNInRadiusSearch(c["q"], k, rad)
        oi, od, oc = orc.knn_batch(tree_o, c["q"], k, rad)
        assert np.array_equal(gc, oc) and np.array_equal(_bits(gd), _bits(od)), (k, rad)
        assert np.array_equal(gi, oi), (k, rad, np.nonzero((gi != oi).any(axis=1))[0][:5])
    for rr in (0.0, np.float32(2.0 * c["h"] ** 2), np.float32(9.0 * c["h"] ** 2)):
        off, idx, d2 = tree_g.radiusSearch(c["q"], rr)
        ooff, oidx, od2 = orc.radius_search(c["dst"], c["q"], rr)
        assert np.array_equal(off, ooff) and np.array_equal(idx, oidx) and np.array_equal(_bits(d2), _bits(od2)), rr
