"""GPU: connected-component segmentation (cilhip_connected_components3f, cilhip_connected_components_lists and their Python / C++ mirrors)
against the numpy restatements of tests/_cc_refs.py (pinned on the CPU by tests/test_components_refs_cpu.py, which also asserts that no
decision of these fixtures sits within 4 ulp of a threshold).  The contract is exact: labels, segment count, offsets and members are
compared with np.array_equal, no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import _cc_refs as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def cl():
    from cilantro_amd import clustering

    return clustering


@pytest.fixture(scope="module")
def frame():
    return R.downsampled_frame()


def evaluator_of(cl, c):
    """the Python mirror's evaluator for a set of clauses (through the class of that name where the reference has one)"""
    ev = cl.AlwaysTrueEvaluator()
    ev.normals, ev.colors, ev.max_distance, ev.max_angle, ev.color_thresh, ev.angle_inclusive = c.normals, c.colors, c.max_distance, c.max_angle, c.color_thresh, c.angle_inclusive
    return ev


def check(cl, p, radius_sq, c=None, ref=None, evaluator=None, **kw):
    """one fused call against the restatement -> the reference arrays"""
    c = c or R.Clauses()
    if ref is None:
        ref = R.fast_components(p, radius_sq, c, **kw)
    kw = dict(kw)
    if kw.get("max_segment_size") is None:
        kw.pop("max_segment_size", None)
    got = cl.connected_components(p, radius_sq, evaluator if evaluator is not None else evaluator_of(cl, c), **kw)
    assert len(got[1]) == len(ref[1]), (len(got[1]) - 1, len(ref[1]) - 1)
    for name, g, r in zip(("labels", "offsets", "members"), got, ref):
        assert np.array_equal(g, r), name
    return ref


# ---- the reference's sensor frame, its example's parameters ----------------------------------------------------------------------
def test_sensor_frame(cl, frame):
    p, nrm, _, _ = frame
    n = p.shape[0]
    r2 = np.float32(0.02 * 0.02)
    ref = check(cl, p, r2, evaluator=cl.NormalsProximityEvaluator(nrm, R.deg(2.0)), ref=R.fast_components(p, r2, R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True),
                                                                                                             min_segment_size=100, max_segment_size=n),
                min_segment_size=100, max_segment_size=n)
    assert np.diff(ref[1]).tolist() == [717, 595, 433, 370, 361, 163, 154, 113]
    ref = check(cl, p, r2, R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True))
    assert len(ref[1]) - 1 == 5127
    ref = check(cl, p, r2, R.Clauses(normals=nrm, max_angle=R.deg(5.0), angle_inclusive=True), min_segment_size=100, max_segment_size=n)
    assert len(ref[1]) - 1 == 6 and ref[1][1] == 9564
    ref = check(cl, p, r2)
    assert np.diff(ref[1]).tolist() == [10548, 2588, 1189, 891, 289, 26]
    # the class, as the example uses it
    cce = cl.ConnectedComponentExtraction3f(p).segment(cl.RadiusNeighborhoodSpecification(r2), cl.NormalsProximityEvaluator(nrm, R.deg(2.0)), 100, n)
    want = R.fast_components(p, r2, R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True), min_segment_size=100)
    assert cce.getNumberOfClusters() == 8 and cce.getNumberOfPoints() == n and np.array_equal(cce.getPointToClusterIndexMap(), want[0])
    segs = cce.getClusterToPointIndicesMap()
    assert [len(s) for s in segs] == np.diff(want[1]).tolist() and all(np.array_equal(s, want[2][want[1][k]:want[1][k + 1]]) for k, s in enumerate(segs))
    assert np.array_equal(cce.getLabeledPointIndices(), np.nonzero(want[0] < 8)[0]) and np.array_equal(cce.getUnlabeledPointIndices(), np.nonzero(want[0] == 8)[0])


def test_every_evaluator_class(cl, frame):
    p, nrm, col, flipped = frame
    r2 = np.float32(0.02 * 0.02)
    seen = {}
    for name, args, c in R.evaluator_cases(nrm, flipped, col):
        ref = check(cl, p, r2, c, evaluator=getattr(cl, name)(*args), min_segment_size=2)
        # (a class with an angle comes twice: the folded angle on the sign-flipped normals decides as the plain one on the frame's)
        assert seen.setdefault(name, len(ref[1]) - 1) == len(ref[1]) - 1
    assert len(seen) == 8 and len(set(seen.values())) == 8      # every clause bites: the classes are told apart by their results
    # <= against <: a threshold that IS a pair's angle joins it in NormalsProximityEvaluator alone
    q = np.array([[0, 0, 0], [0.01, 0, 0]], np.float32)
    nn = np.array([[0, 0, 1], [0, 0.6, 0.8]], np.float32)
    a = R.pair_angle(nn, np.array([0]), np.array([1]))[0]
    assert cl.connected_components(q, 1.0, cl.NormalsProximityEvaluator(nn, a))[0].tolist() == [0, 0]
    assert cl.connected_components(q, 1.0, cl.PointsNormalsProximityEvaluator(nn, 1.0, a))[0].tolist() == [0, 1]
    assert cl.connected_components(q, 1.0, cl.NormalsProximityEvaluator(nn, np.nextafter(a, np.float32(0))))[0].tolist() == [0, 1]


def test_equal_sizes_are_ordered_by_lowest_member(cl, frame):
    p, nrm, _, _ = frame
    ref = check(cl, p, np.float32(0.01 * 0.01), R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True), min_segment_size=10)
    sizes = np.diff(ref[1])
    assert len(sizes) == 189 and int((np.diff(sizes) == 0).sum()) == 136
    low = ref[2][ref[1][:-1]]      # every segment's lowest member
    tie = np.diff(sizes) == 0
    assert (np.diff(low)[tie] > 0).all()


def test_raw_frame(cl):
    """120 111 points, mean degree about 32: more than one block of every kernel, real over-long normals (dot > 1 -> NaN -> not similar)"""
    P, N = R.raw_frame()
    r2 = np.float32(R.RAW_RADIUS ** 2)
    ref = check(cl, P, r2, R.Clauses(normals=N, max_angle=R.deg(5.0), angle_inclusive=True), min_segment_size=50)
    assert len(ref[1]) - 1 > 5
    check(cl, P, r2, min_segment_size=2, max_segment_size=20000)


# ---- chains: the deepest trees the hook can build ----------------------------------------------------------------------------------
def chain_check(cl, p, r2, root, c=None):
    ref = R.finish(p.shape[0], root)
    return check(cl, p, r2, c, ref=ref)


def test_chains(cl):
    n = 100_000
    p, pos = R.chain(n, 0.9, 1.0)
    ref = chain_check(cl, p, np.float32(1.0), R.chain_roots(p, np.float32(1.0)))
    assert len(ref[1]) - 1 == 1 and (ref[0] == 0).all()
    g, gpos = R.chain(n, 0.9, 1.0, gap_at=40_000, gap=1.1)
    ref = chain_check(cl, g, np.float32(1.0), R.chain_roots(g, np.float32(1.0)))
    assert np.diff(ref[1]).tolist() == [59_999, 40_001]
    # every second normal along the line turned by 90 degrees: no two neighbours are similar
    nrm = np.zeros((n, 3), np.float32)
    nrm[pos % 2 == 0, 2] = 1
    nrm[pos % 2 == 1, 0] = 1
    c = R.Clauses(normals=nrm, max_angle=R.deg(10.0), angle_inclusive=True)
    ref = chain_check(cl, p, np.float32(1.0), np.arange(n), c)
    assert len(ref[1]) - 1 == n and np.array_equal(ref[0], np.arange(n))
    # ... and turned by less than the threshold: one segment again
    nrm[pos % 2 == 1] = np.array([np.sin(0.1), 0, np.cos(0.1)], np.float32)
    ref = chain_check(cl, p, np.float32(1.0), R.chain_roots(p, np.float32(1.0)), R.Clauses(normals=nrm, max_angle=R.deg(10.0), angle_inclusive=True))
    assert len(ref[1]) - 1 == 1


def test_chain_past_one_trip_of_the_strided_kernels(cl):
    """600 001 points (the grid-stride kernels of the chain cover 524 288 per trip), four gaps: five segments of different sizes"""
    n = 600_001
    x = np.arange(n, dtype=np.float64) * 0.75
    for k, at in enumerate((50_000, 170_000, 300_000, 599_000)):
        x[at + 1:] += 0.5 + 0.25 * k
    pos = np.random.default_rng(5).permutation(n)
    p = np.zeros((n, 3), np.float32)
    p[:, 0] = x[pos].astype(np.float32)
    assert np.array_equal(p[:, 0].astype(np.float64), x[pos])      # exactly representable
    ref = chain_check(cl, p, np.float32(1.0), R.chain_roots(p, np.float32(1.0)))
    assert sorted(np.diff(ref[1]).tolist()) == sorted([50_001, 120_000, 130_000, 299_000, 1000])


# ---- single rules, each on its own small cloud ---------------------------------------------------------------------------------------
def over_long_normal():
    """(0.6, 0.8, 0) pushed up by a few ulps until its f32 self dot product rounds above 1"""
    v = np.array([0.6, 0.8, 0.0], np.float32)
    for _ in range(8):
        if R.dot_pinned(v, v) > 1:
            return v
        v[:2] = np.nextafter(v[:2], np.float32(2))
    raise AssertionError("no over-long normal found")


def test_dot_product_above_one_is_not_similar(cl):
    v = over_long_normal()
    assert R.dot_pinned(v, v) > np.float32(1) and np.isnan(R.pair_angle(v[None], np.array([0]), np.array([0]))[0])
    p = np.array([[0, 0, 0], [0.01, 0, 0], [5, 0, 0], [5.01, 0, 0]], np.float32)
    nrm = np.array([v, v, [0.6, 0.8, 0], [0.6, 0.8, 0]], np.float32)
    assert R.dot_pinned(nrm[2], nrm[3]) <= np.float32(1)
    for ev, c in ((cl.NormalsProximityEvaluator(nrm, 0.5), R.Clauses(normals=nrm, max_angle=0.5, angle_inclusive=True)),
                  (cl.NormalsProximityEvaluator(nrm, -0.5), R.Clauses(normals=nrm, max_angle=-0.5, angle_inclusive=True)),
                  (cl.PointsNormalsProximityEvaluator(nrm, 1.0, 0.5), R.Clauses(normals=nrm, max_distance=1.0, max_angle=0.5))):
        ref = check(cl, p, np.float32(1.0), c, evaluator=ev)
        assert ref[0].tolist() == [1, 2, 0, 0]      # the two identical over-long normals are not joined, the unit ones are


def test_duplicates_non_finite_points_and_degenerate_radii(cl):
    rng = np.random.default_rng(21)
    base = rng.random((300, 3), dtype=np.float32)
    p = np.concatenate([base, base[:100], base[:50]])[rng.permutation(450)]
    nrm = np.tile(np.array([0, 0, 1], np.float32), (450, 1))
    # exact duplicates are joined (d2 = 0 < radius_sq), whichever comes first in a list
    tiny = np.float32(1e-12)
    ref = check(cl, p, tiny, R.Clauses(normals=nrm, max_angle=R.deg(1.0), angle_inclusive=True))
    assert sorted(np.diff(ref[1]).tolist(), reverse=True) == [3] * 50 + [2] * 50 + [1] * 200
    # a point with a non-finite coordinate is a singleton, wherever it is; the others are unaffected
    q = p.copy()
    bad = [0, 17, 449]
    q[0, 1], q[17, 0], q[449, 2] = np.nan, np.inf, -np.inf
    ref = check(cl, q, np.float32(0.2 * 0.2))
    sizes = np.bincount(ref[0])
    assert all(sizes[ref[0][b]] == 1 for b in bad) and sizes.max() > 100
    check(cl, np.full((70, 3), np.nan, np.float32), np.float32(1.0))
    check(cl, q[:1], np.float32(1.0))
    check(cl, p[:1], np.float32(1.0))
    # radius_sq <= 0: every point a singleton (duplicates too); equal sizes by lowest member: labels are the indices
    for r2 in (0.0, -1.0):
        got = cl.connected_components(p, r2)
        assert np.array_equal(got[0], np.arange(450)) and np.array_equal(got[1], np.arange(451)) and np.array_equal(got[2], np.arange(450))


def test_seeds_size_limits_and_the_unlabelled_label(cl, frame):
    p, nrm, _, _ = frame
    n = p.shape[0]
    r2 = np.float32(0.02 * 0.02)
    c = R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True)
    full = R.fast_components(p, r2, c)
    sizes = np.diff(full[1])
    rng = np.random.default_rng(31)
    seeds = rng.permutation(n)[:40]
    for kw in ({"seeds": seeds}, {"seeds": seeds, "min_segment_size": 3}, {"seeds": np.concatenate([seeds, seeds])}, {"seeds": np.zeros(0, np.int64)},
               {"min_segment_size": 154, "max_segment_size": 595}, {"min_segment_size": 155, "max_segment_size": 594}, {"max_segment_size": 1}, {"min_segment_size": n}):
        ref = check(cl, p, r2, c, **kw)
        k = len(ref[1]) - 1
        assert ref[0].max() == k or k == len(sizes)      # the unlabelled label is the segment count
        assert (np.bincount(ref[0], minlength=k + 1)[:k] == np.diff(ref[1])).all()
    # a segment one past the maximum is dropped whole; a seed inside a dropped segment labels nothing
    big = int(sizes[0])
    ref = check(cl, p, r2, c, max_segment_size=big - 1)
    assert len(ref[1]) - 1 == len(sizes) - 1 and ref[1][1] == sizes[1]
    seed_in_big = full[2][:1]
    ref = check(cl, p, r2, c, seeds=seed_in_big, max_segment_size=big - 1)
    assert len(ref[1]) - 1 == 0 and (ref[0] == 0).all()
    ref = check(cl, p, r2, c, seeds=seed_in_big, max_segment_size=big)
    assert np.diff(ref[1]).tolist() == [big]
    from cilantro_amd import capi

    with pytest.raises(capi.CilhipError) as ei:
        cl.connected_components(p, r2, seeds=[n])
    assert ei.value.code == capi.ERR_INVALID


def test_device_tensors_in_device_tensors_out(cl, frame):
    import torch

    p, nrm, col, _ = frame
    r2 = np.float32(0.02 * 0.02)
    tp, tn, tc = (torch.from_numpy(x).cuda() for x in (p, nrm, col))
    for host_ev, dev_ev, kw in ((cl.NormalsProximityEvaluator(nrm, R.deg(2.0)), cl.NormalsProximityEvaluator(tn, R.deg(2.0)), {"min_segment_size": 100}),
                                (cl.PointsNormalsColorsProximityEvaluator(nrm, col, r2 * 0.7, -R.deg(8.0), 0.8), cl.PointsNormalsColorsProximityEvaluator(tn, tc, r2 * 0.7, -R.deg(8.0), 0.8),
                                 {"min_segment_size": 2, "seeds": np.arange(0, p.shape[0], 5)}),
                                (None, None, {})):
        host = cl.connected_components(p, r2, host_ev, **kw)
        dev = cl.connected_components(tp, r2, dev_ev, **kw)
        assert all(isinstance(h, np.ndarray) for h in host) and all(d.is_cuda for d in dev)
        assert all(np.array_equal(h, d.cpu().numpy()) for h, d in zip(host, dev)) and len(host[1]) > 3
    cce = cl.ConnectedComponentExtraction3f(tp).segment(cl.RadiusNeighborhoodSpecification(r2), cl.NormalsProximityEvaluator(tn, R.deg(2.0)), 100, p.shape[0])
    assert cce.getNumberOfClusters() == 8 and cce.getPointToClusterIndexMap().is_cuda and cce.getClusterToPointIndicesMap()[0].shape[0] == 717
    assert cce.getLabeledPointIndices().shape[0] + cce.getUnlabeledPointIndices().shape[0] == p.shape[0]
    with pytest.raises(ValueError):
        cl.connected_components(tp, r2, cl.NormalsProximityEvaluator(nrm, 0.1))      # one memory space per call


# ---- the lists entry --------------------------------------------------------------------------------------------------------------
def test_lists_entry(cl, frame):
    import torch
    from cilantro_amd import capi
    from cilantro_amd.normal_estimation import KDTree3f

    p, nrm, _, _ = frame
    n = p.shape[0]
    r2 = np.float32(0.02 * 0.02)
    tree = KDTree3f(p)
    off, idx, d2 = tree.radiusSearch(None, r2)
    assert idx.size == 954198 + n and (idx[off[:-1]] == np.arange(n)).all()      # 477 099 pairs from both ends, and every list starts with its own point
    # radius lists with skip_first reproduce the fused call
    got = cl.connected_components_from_lists(n, off, idx, skip_first=True, min_segment_size=20)
    want = R.fast_components(p, r2, min_segment_size=20)
    ref = R.components_from_lists(n, off, idx, skip_first=True, min_segment_size=20)
    assert all(np.array_equal(g, w) and np.array_equal(g, r) for g, w, r in zip(got, want, ref))
    # a byte mask: the caller's own evaluator, applied on the host
    c = R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True)
    src = np.repeat(np.arange(n), np.diff(off))
    keep = R.similar(c, src, idx, d2).astype(np.uint8)
    seeds = np.arange(0, n, 11)
    for kw in ({"min_segment_size": 100}, {"seeds": seeds, "min_segment_size": 2, "max_segment_size": 400}):
        got = cl.connected_components_from_lists(n, off, idx, keep=keep, skip_first=True, **kw)
        want = R.fast_components(p, r2, c, **kw)
        ref = R.components_from_lists(n, off, idx, keep=keep, skip_first=True, **kw)
        assert all(np.array_equal(g, w) and np.array_equal(g, r) for g, w, r in zip(got, want, ref)), kw
    dev = cl.connected_components_from_lists(n, torch.from_numpy(off).cuda(), torch.from_numpy(idx).cuda(), keep=torch.from_numpy(keep).cuda(), min_segment_size=100)
    assert all(d.is_cuda and np.array_equal(d.cpu().numpy(), w) for d, w in zip(dev, R.fast_components(p, r2, c, min_segment_size=100)))
    # k-NN lists (k = 8, the cloud against itself) are directed: the weak components
    kidx, _, cnt = tree.kNNSearch(None, 8)
    flat = np.where(kidx < 0, capi.NONE_IDX, kidx).astype(np.uint32).reshape(-1)
    koff = np.arange(n + 1, dtype=np.int64) * 8
    edges = set(zip(np.repeat(np.arange(n), 7).tolist(), kidx[:, 1:].reshape(-1).tolist()))
    assert any((b, a) not in edges for a, b in edges) and (cnt == 8).all() and (kidx[:, 0] == np.arange(n)).all()
    for skip in (True, False):
        got = cl.connected_components_from_lists(n, koff, flat, skip_first=skip, symmetric=False, min_segment_size=2)
        ref = R.components_from_lists(n, koff, flat, skip_first=skip, min_segment_size=2)
        assert all(np.array_equal(g, r) for g, r in zip(got, ref)) and len(ref[1]) > 2
    short = np.where(np.arange(8)[None, :] < 4, kidx, -1)      # rows padded with NONE: the padding is no neighbour
    flat4 = np.where(short < 0, capi.NONE_IDX, short).astype(np.uint32).reshape(-1)
    got = cl.connected_components_from_lists(n, koff, flat4, skip_first=False, symmetric=False)
    assert all(np.array_equal(g, r) for g, r in zip(got, R.components_from_lists(n, koff, flat4, skip_first=False)))
    with pytest.raises(capi.CilhipError) as ei:
        cl.connected_components_from_lists(n, koff, flat, symmetric=False, seeds=[0])
    assert ei.value.code == capi.ERR_UNSUPPORTED


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_gives_the_python_mirror_labels(cl, frame, tmp_path):
    from cilantro_amd import ply_io
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_components.cpp"), "test_components")
    p, nrm, col, flipped = frame
    rng = np.random.default_rng(41)
    q, nn = p.copy(), flipped.copy()
    bad_p, bad_n = rng.permutation(p.shape[0])[:60], rng.permutation(p.shape[0])[:40]
    q[bad_p, rng.integers(0, 3, 60)] = np.nan
    nn[bad_n, rng.integers(0, 3, 40)] = np.inf
    q[-1] = np.nan      # the last row too: the compaction looks for the last row that stays
    ply = str(tmp_path / "frame.ply")
    ply_io.write_ply(ply, q, nn, col)
    pre = str(tmp_path / "out")
    r = subprocess.run([exe, "run", ply, pre, "0.02", "5", "20"], capture_output=True, text=True)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
    P, N, Cc = (np.fromfile(f"{pre}.{a}.f32", np.float32).reshape(-1, 3) for a in "pnc")
    ok = np.isfinite(q).all(axis=1) & np.isfinite(nn).all(axis=1)
    assert P.shape[0] == int(ok.sum()) < p.shape[0] - 90 and np.isfinite(P).all() and np.isfinite(N).all()
    as_rows = lambda a: sorted(map(bytes, np.ascontiguousarray(a)))      # noqa: E731
    assert as_rows(np.hstack([P, N])) == as_rows(np.hstack([q[ok], nn[ok]]))      # the same rows, in the reference's (not the input's) order
    n = P.shape[0]
    r2 = np.float32(0.02) * np.float32(0.02)
    a = R.deg(5.0)
    lab = lambda v: np.fromfile(f"{pre}.{v}.u64", np.uint64).astype(np.int64)      # noqa: E731
    assert np.array_equal(lab("normals"), cl.connected_components(P, r2, cl.NormalsProximityEvaluator(N, a), 20, n)[0])
    assert np.array_equal(lab("seeded"), cl.connected_components(P, r2, cl.NormalsProximityEvaluator(N, a), 2, seeds=np.arange(0, n, 7))[0])
    assert np.array_equal(lab("pnc"), cl.connected_components(P, r2, cl.PointsNormalsColorsProximityEvaluator(N, Cc, np.float32(0.6) * np.float32(0.02) * np.float32(0.02), -a, np.float32(0.7)), 3, 500)[0])
    assert np.array_equal(lab("plain"), cl.connected_components(P, r2)[0])
    assert len(set(lab("normals").tolist())) > 3 and len(set(lab("pnc").tolist())) > 3
