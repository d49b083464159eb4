"""The kernels around the ICP loop -- kmeans.hip, ransac.hip, ransac_transform.hip, the list and moment kernels of knn.hip -- at
the sizes where their launch code takes another path than the one the other exact tests reach, and off the origin.

  * KMeans: the cluster sums are documented as EXACT fixed-point integers (scale 2^S) and the product exposes them
    (HipKMeansShard.assign), so they are compared with an integer reference (tests/_model_refs.py, pinned on the CPU against
    rational arithmetic) for equality: cloud sizes around the pair kernel's tail (odd n, n = 1), a multiple of 256 and the
    grid-stride trips (n > 524 288, n > 1 048 576), k around the 8-centroid blocks, the grid's floor (64) and the LDS limit (2048),
    pruning on and off, both distance roundings, clouds rescaled so that S leaves 0..63, moved off the origin and across zero,
    exact ties on either side of the tie list's capacity, the empty-cluster repair, Lloyd runs step by step, non-finite points;
  * RANSAC: inlier counts of 1..257 planes / 1..129 transforms with a NaN hypothesis in every round, at cloud sizes around a tile,
    around the first chunk carry of the ordered inlier list and past the first grid trip of the scoring kernel; whole runs there
    with the residuals bit for bit and the inlier list element for element; rescaled and moved clouds; clouds of 0-3 points;
  * radius lists and normals on clouds moved off the origin, k = 32 / 33.
Every test writes its counts as model_kernels_*.json (_report)."""
import time

import numpy as np
import pytest

import _model_refs as mr
from cilantro_amd import capi
from test_gpu_cloud_frames import _moved
from test_gpu_parity import _kmeans_label_mismatches_are_near_ties, _plane_cloud, _report

pytestmark = pytest.mark.gpu


def _mv(x, scale=1.0, offset=0.0):
    """one cloud through _moved (f64 scale and offset, rounded once to f32)"""
    return _moved({"dst": x, "dst_n": None, "src": x[:1], "max_sq_dist": 1.0}, scale=scale, offset=offset)["dst"]


@pytest.fixture(scope="module")
def cloud():
    """1 300 001 points: a mixture of 40 blobs in the unit cube (k-means has structure) -- every KMeans size is a prefix of it"""
    rng = np.random.default_rng(71)
    centres = rng.random((40, 3))
    x = centres[rng.integers(0, 40, 1_300_001)] + rng.normal(0, 0.03, (1_300_001, 3))
    return np.ascontiguousarray(np.clip(x, 0.0, 0.999).astype(np.float32))


def _start_centroids(x, k):
    """k distinct points of the cloud, spread over it"""
    idx = (np.arange(k, dtype=np.int64) * len(x)) // k
    return np.ascontiguousarray(x[idx])


def _shard_pass(x, cents, kd, S, want_labels, prev=None, offset=0, refs=None):
    """HipKMeansShard over x: one assign() per centroid set in `cents`, each against the oracle's labels (want_labels[i]) and the
    integer reference under them; `changed` against the previous call's labels (first call: zeros) -> list of failure tuples"""
    from cilantro_amd.distributed_models import HipKMeansShard

    bad = []
    k = len(cents[0])
    sh = HipKMeansShard(x, k, index_offset=offset)
    try:
        prev = np.zeros(len(x), np.int64) if prev is None else prev
        for i, c in enumerate(cents):
            sums, changed = sh.assign(c, S, use_kd_tree=kd)
            lab = sh.labels()
            want = want_labels[i]
            nlab = int(np.count_nonzero(lab != want))
            if nlab:
                bad.append(("labels", i, nlab, np.nonzero(lab != want)[0][:5].tolist()))
            ref = mr.kmeans_sums(x, want, k, S) if refs is None else refs[i]
            if not np.array_equal(sums, ref):
                rows = np.nonzero((sums != ref).any(axis=1))[0]
                bad.append(("sums", i, len(rows), rows[:4].tolist(), sums[rows[:2]].tolist(), ref[rows[:2]].tolist()))
            want_changed = int(np.count_nonzero(want != prev))
            if changed != want_changed:
                bad.append(("changed", i, changed, want_changed))
            prev = want
    finally:
        sh.close()
    return bad


KM_SIZES = (1, 2, 3, 255, 256, 257, 511, 513, 524_287, 524_288, 524_289, 1_048_575, 1_048_577, 1_300_001)
KM_KS = (1, 7, 8, 9, 63, 64, 65, 2047, 2048)


def _size_cases():
    cases = []
    for n in KM_SIZES:
        for k in (7, 64, 1024):
            cases.append((n, min(k, n)))
    for k in KM_KS:
        for n in (524_287, 1_048_577):
            cases.append((n, k))
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


def test_kmeans_integer_sums_at_tail_and_trip_sizes(orc, hip_lib, cloud):
    """assign(c, S) through the shard handle: labels equal the oracle's element for element, the int64 sums and counts equal the
    integer reference's, `changed` counts the labels that differ from the previous call's (first call: from zeros) -- n at the
    pair tail (odd, 1), at multiples of 256 +- 1 and on either side of each grid-stride trip of both assignment kernels; k around
    the blocks of 8 centroids, the grid's floor and the LDS limit; pruning on and off; both distance roundings.  Two calls per
    handle for k <= 65 (the second under the centroids in reverse order: nearly every label changes)."""
    from cilantro_amd import clustering
    from cilantro_amd.clustering import kmeans_assign

    failures = []
    report = {"cases": 0, "handles": 0}
    t0 = time.time()
    try:
        for n, k in _size_cases():
            x = np.ascontiguousarray(cloud[:n])
            S = mr.scale_for(x)
            c1 = _start_centroids(x, k)
            cents = [c1, np.ascontiguousarray(c1[::-1])] if k <= 65 else [c1]
            for kd in (False, True):
                want = [orc.kmeans_assign(x, c, use_kd_tree=kd)[0] for c in cents]
                refs = [mr.kmeans_sums(x, w, k, S) for w in want]
                for prune in (True, False):
                    clustering.set_pruning(prune)
                    bad = _shard_pass(x, cents, kd, S, want, refs=refs)
                    lab = kmeans_assign(x, c1, use_kd_tree=kd)
                    if not np.array_equal(lab, want[0]):
                        bad.append(("kmeans_assign labels", int(np.count_nonzero(lab != want[0]))))
                    report["handles"] += 1
                    if bad:
                        failures.append((n, k, "kd" if kd else "brute", "pruned" if prune else "exhaustive", bad))
            report["cases"] += 1
    finally:
        clustering.set_pruning(True)
    report["seconds"] = round(time.time() - t0, 1)
    report["failures"] = [str(f)[:600] for f in failures]
    _report("model_kernels_kmeans_sizes.json", report)
    assert not failures, failures[:5]


def test_kmeans_rejects_more_than_2048_clusters(hip_lib, cloud):
    from cilantro_amd.clustering import KMeans3f, kmeans_assign
    from cilantro_amd.distributed_models import HipKMeansShard

    x = np.ascontiguousarray(cloud[:5000])
    c = np.ascontiguousarray(x[:2049])
    with pytest.raises(capi.CilhipError) as e:
        KMeans3f(x).cluster(c.copy(), max_iter=1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.CilhipError) as e:
        kmeans_assign(x, c)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.CilhipError) as e:
        HipKMeansShard(x, 2049)
    assert e.value.code == capi.ERR_UNSUPPORTED
    KMeans3f(x).cluster(np.ascontiguousarray(x[:2048]).copy(), max_iter=1)
    _report("model_kernels_kmeans_limit.json", {"k = 2049 refused by": ["cilhip_kmeans3f_ex", "cilhip_kmeans3f_assign_ex", "cilhip_kmeans_shard_create"], "k = 2048 runs": True})


KM_FRAMES = (("identity", 1.0, 0.0), ("x 2^-24", 2.0 ** -24, 0.0), ("x 2^44", 2.0 ** 44, 0.0), ("at (1e3, -250, 37)", 1.0, (1e3, -250.0, 37.0)),
             ("at 4096", 1.0, 4096.0), ("at 16384", 1.0, 16384.0), ("extent 1e3 across zero", 1e3, -500.0), ("all-negative octant", 1.0, -2.0))


def test_kmeans_integer_sums_in_other_frames(orc, hip_lib, cloud):
    """The same equalities on 600 001 points (a second trip of the pair kernel) rescaled by 2^-24 (S above 63: 2^S is still a
    finite double) and 2^44 (S negative; squared distances near 2^90 are finite) -- labels those of the unscaled cloud --, moved
    to (1e3, -250, 37), 4096 and 16384, stretched to an extent of 1e3 across zero (negative coordinates, low bits lost to the
    scale: the reference rounds the same way) and into the all-negative octant; k = 7 (pair kernel) and 64, 257 (grid kernel)."""
    from cilantro_amd import clustering

    base = np.ascontiguousarray(cloud[:600_001])
    failures = []
    report = {}
    unit_labels = {}
    try:
        for name, scale, off in KM_FRAMES:
            x = _mv(base, scale, off)
            S = mr.scale_for(x)
            report[name] = {"S": S, "handles": 0}
            sh_max = None
            for k in (7, 64, 257):
                c1 = _start_centroids(x, k)
                cents = [c1, np.ascontiguousarray(c1[::-1])]
                for kd in (False, True):
                    want = [orc.kmeans_assign(x, c, use_kd_tree=kd)[0] for c in cents]
                    if name == "identity":
                        unit_labels[(k, kd)] = want[0]
                    elif name.startswith("x 2^") and not np.array_equal(want[0], unit_labels[(k, kd)]):
                        failures.append((name, k, kd, "the oracle's labels are not the unscaled cloud's"))
                    refs = [mr.kmeans_sums(x, w, k, S) for w in want]
                    for prune in (True, False):
                        clustering.set_pruning(prune)
                        bad = _shard_pass(x, cents, kd, S, want, refs=refs)
                        report[name]["handles"] += 1
                        if bad:
                            failures.append((name, k, "kd" if kd else "brute", "pruned" if prune else "exhaustive", bad))
            from cilantro_amd.distributed_models import HipKMeansShard
            sh = HipKMeansShard(x, 7)
            sh_max = sh.maxabs()
            sh.close()
            if sh_max != float(np.abs(x).max()):
                failures.append((name, "maxabs", sh_max, float(np.abs(x).max())))
    finally:
        clustering.set_pruning(True)
    assert report["x 2^-24"]["S"] > 63 and report["x 2^44"]["S"] < 0, report
    report["failures"] = [str(f)[:600] for f in failures]
    _report("model_kernels_kmeans_frames.json", report)
    assert not failures, failures[:5]


def _kd_tied_points(x, c):
    """points whose smallest kd-rounded distance ((dx*dx + dy*dy) + dz*dz, f32) is met on two or more centroids"""
    tied = 0
    for lo in range(0, len(x), 20_000):
        p = x[lo:lo + 20_000]
        d = c[None, :, :] - p[:, None, :]
        sq = d * d
        dist = (sq[:, :, 0] + sq[:, :, 1]) + sq[:, :, 2]
        tied += int(np.count_nonzero((dist == dist.min(axis=1, keepdims=True)).sum(axis=1) > 1))
    return tied


def test_kmeans_kd_branch_with_exact_ties_on_either_side_of_the_tie_list(orc, hip_lib, cloud):
    """use_kd_tree with duplicated centroids: (a) twelve of 512 duplicated -- fewer tied points than the tie list holds, the
    pruned pass corrects them in place (labels, both clusters' sums, `changed`); (b) every centroid duplicated -- every point
    ties, the pass runs again with the order tables.  Labels against the oracle's kd branch, sums the integer reference's under
    those final labels, `changed` the final count; a second call on the same handle (the duplicates moved) so that `changed` is
    counted against real previous labels.  Pruning off: the rerun path in both."""
    from cilantro_amd import clustering

    x = np.ascontiguousarray(cloud[:300_001])
    S = mr.scale_for(x)
    base = _start_centroids(x, 512)
    a1 = base.copy(); a1[500:512] = a1[0:12]
    a2 = base.copy(); a2[488:500] = a2[20:32]
    b1 = base.copy(); b1[256:] = b1[:256]
    b2 = base.copy(); b2[:256] = b2[256:]
    report = {}
    failures = []
    try:
        for name, cents in (("a: 12 duplicated", [a1, a2]), ("b: all duplicated", [b1, b2])):
            tied = [_kd_tied_points(x, c) for c in cents]
            report[name] = {"tied points": tied}
            if name[0] == "a":
                assert 0 < max(tied) < 65_536, tied
            else:
                assert min(tied) > 65_536, tied
            want = [orc.kmeans_assign(x, c, use_kd_tree=True)[0] for c in cents]
            report[name]["labels that are not the lowest index"] = [int(np.count_nonzero(w != orc.kmeans_assign(x, c)[0])) for w, c in zip(want, cents)]
            for prune in (True, False):
                clustering.set_pruning(prune)
                bad = _shard_pass(x, cents, True, S, want)
                if bad:
                    failures.append((name, "pruned" if prune else "exhaustive", bad))
    finally:
        clustering.set_pruning(True)
    report["failures"] = [str(f)[:600] for f in failures]
    _report("model_kernels_kmeans_ties.json", report)
    assert not failures, failures


def test_kmeans_farthest_member_and_move_point(orc, hip_lib, cloud):
    """farthest(cluster, centre) against numpy: key = bits(d) << 32 | (0xFFFFFFFF - global index), d the pinned
    d0*d0 + (d1*d1 + d2*d2); every point of the cloud twice, so every maximum is met on two indices and the lower one is named;
    0 for an empty cluster; a non-zero index offset.  move_point returns the point and labels() shows it moved."""
    from cilantro_amd.distributed_models import HipKMeansShard

    half = np.ascontiguousarray(cloud[:300_001])
    x = np.ascontiguousarray(np.concatenate([half, half]))
    k, off = 9, 1_000_003
    c = _start_centroids(half, k); c[4] = [50.0, 50.0, 50.0]
    S = mr.scale_for(x)
    lab, _ = orc.kmeans_assign(x, c)
    assert np.count_nonzero(lab == 4) == 0
    sh = HipKMeansShard(x, k, index_offset=off)
    report = {"clusters": k, "mismatches": 0}
    try:
        sh.assign(c, S)
        assert np.array_equal(sh.labels(), lab)
        for j in range(k):
            for centre in (c[j], c[(j + 1) % k], np.float32([0.5, 0.5, 0.5])):
                got, want = sh.farthest(j, centre), mr.farthest_key(x, lab, j, centre, off)
                report["mismatches"] += got != want
                assert got == want, (j, hex(got), hex(want))
                if j != 4:
                    assert 0xFFFFFFFF - (got & 0xFFFFFFFF) - off < len(half)      # (the lower of the two equal points)
        assert sh.farthest(4, c[4]) == 0
        g = off + 123_457
        p = sh.move_point(g, 4)
        assert np.array_equal(p.view(np.uint32), x[123_457].view(np.uint32))
        lab2 = lab.copy(); lab2[123_457] = 4
        assert np.array_equal(sh.labels(), lab2)
        assert sh.farthest(4, np.float32([0, 0, 0])) == mr.farthest_key(x, lab2, 4, np.float32([0, 0, 0]), off)
        for outside in (off - 1, off + len(x)):
            with pytest.raises(capi.CilhipError):
                sh.move_point(outside, 0)
    finally:
        sh.close()
    _report("model_kernels_kmeans_farthest.json", report)


def _lloyd_frames(cloud):
    base = np.ascontiguousarray(cloud[:600_001])
    return (("unit", base), ("at 4096", _mv(base, 1.0, 4096.0)), ("extent 1e3 across zero", _mv(base, 1e3, -500.0)))


@pytest.mark.parametrize("which", range(3))
def test_kmeans_lloyd_steps_one_at_a_time(orc, hip_lib, cloud, which):
    """Eight Lloyd steps, each run by the product for ONE iteration from the oracle's centroids after the step before (so that a
    last-bit difference cannot grow into another trajectory): labels identical to the oracle's assignment + the repair restated
    on the integers, centroids bit-identical to the integer reference's -- through cilhip_kmeans3f and through the shard loop
    (ShardedKMeans3f over HipKMeansShard), which must agree.  k = 64 (grid kernel) and k = 8 with one initial centroid far away
    (the empty-cluster repair runs in step 0).  Then one free run of 8 iterations against the oracle under the existing
    contract, centroids within max(1e-6, one ulp)."""
    from cilantro_amd.clustering import KMeans3f
    from cilantro_amd.distributed_models import HipKMeansShard, ShardedKMeans3f

    name, x = _lloyd_frames(cloud)[which]
    S = mr.scale_for(x)
    report = {"frame": name, "S": S}
    failures = []
    for k, far in ((64, False), (8, True)):
        cent = _start_centroids(x, k)
        if far:
            cent[5] = cent[5] + np.float32(50.0 * float(x.max() - x.min()))      # fifty extents away: attracts nothing
        c0 = cent.copy()
        differ_from_oracle = 0
        repairs = 0
        for t in range(8):
            lab_a, _ = orc.kmeans_assign(x, cent)
            repairs += int(np.count_nonzero(np.bincount(lab_a, minlength=k) == 0))
            want_c, want_l, _ = mr.lloyd_step(x, lab_a, cent, S)
            km = KMeans3f(x).cluster(cent.copy(), max_iter=1, tol=0.0)
            sh = HipKMeansShard(x, k)
            sk = ShardedKMeans3f(sh).cluster(cent.copy(), max_iter=1, tol=0.0)
            sh.close()
            for pname, got in (("cilhip_kmeans3f", km), ("shard loop", sk)):
                gc, gl = got.getClusterCentroids(), got.getPointToClusterIndexMap()
                if got.getNumberOfPerformedIterations() != 1:
                    failures.append((k, t, pname, "iterations", got.getNumberOfPerformedIterations()))
                if not np.array_equal(gl, want_l):
                    failures.append((k, t, pname, "labels", int(np.count_nonzero(gl != want_l))))
                if not np.array_equal(gc.view(np.uint32), want_c.view(np.uint32)):
                    failures.append((k, t, pname, "centroids", int(np.count_nonzero(gc.view(np.uint32) != want_c.view(np.uint32)))))
            co, lo, _ = orc.kmeans(x, cent, max_iter=1, tol=0.0, mode=1)
            differ_from_oracle += int(np.count_nonzero(co.view(np.uint32) != want_c.view(np.uint32)))
            cent = co
        report[f"k={k}/integer reference's coordinates that differ from the oracle's f64 sums, 8 steps"] = differ_from_oracle
        report[f"k={k}/empty clusters repaired"] = repairs
        if far and repairs == 0:
            failures.append((k, "the far centroid attracted points: no repair ran"))
        # free run
        km = KMeans3f(x).cluster(c0.copy(), max_iter=8, tol=0.0)
        co, lo, ito = orc.kmeans(x, c0, max_iter=8, tol=0.0, mode=1)
        gc = km.getClusterCentroids()
        report[f"k={k}/free run: coordinates not bit-identical"] = int(np.count_nonzero(gc.view(np.uint32) != co.view(np.uint32)))
        report[f"k={k}/free run: labels differing"] = int(np.count_nonzero(km.getPointToClusterIndexMap() != lo))
        if km.getNumberOfPerformedIterations() != ito:
            failures.append((k, "free run iterations", km.getNumberOfPerformedIterations(), ito))
        tol = np.maximum(1e-6, np.spacing(np.abs(co)).astype(np.float64))
        err = np.abs(gc.astype(np.float64) - co.astype(np.float64))
        if not (err <= tol).all():
            failures.append((k, "free run centroids", float((err / tol).max())))
        _kmeans_label_mismatches_are_near_ties(x, km.getPointToClusterIndexMap(), lo, co, k)
    report["failures"] = [str(f) for f in failures]
    _report(f"model_kernels_kmeans_lloyd_{which}.json", report)
    assert not failures, failures[:6]


def test_kmeans_run_with_non_finite_points(orc, hip_lib, cloud):
    """A NaN point and a +inf point in a Lloyd run of 1 and 3 iterations, k = 8 (pair kernel) and 64 (grid kernel), brute and kd (one iteration),
    single-device entry and shard loop, against orc.kmeans(mode=1): the same labels, NaN exactly where the oracle has NaN, every
    other coordinate of every centroid bit-identical (the two points fall into cluster 0: the other clusters must not notice)."""
    from cilantro_amd.clustering import KMeans3f
    from cilantro_amd.distributed_models import HipKMeansShard, ShardedKMeans3f

    failures = []
    report = {"cases": 0}
    for n, shift in ((20_001, 0.0), (600_001, 0.0), (20_001, 4096.0)):
        x = _mv(np.ascontiguousarray(cloud[:n]), 1.0, shift)
        x[17] = [np.nan, x[17, 1], x[17, 2]]
        x[n // 2] = [x[n // 2, 0], np.inf, x[n // 2, 2]]
        for k in (8, 64):
            c0 = _start_centroids(x[1000:], k)
            for kd in (False, True):
                # (kd branch: one iteration only -- after it centroid 0 is NaN, and a kd-tree built over a NaN centroid is not defined)
                for iters in ((1,) if kd else (1, 3)):
                    co, lo, ito = orc.kmeans(x, c0, max_iter=iters, tol=0.0, mode=1, use_kd_tree=kd)
                    assert lo[17] == 0 and lo[n // 2] == 0 and np.isnan(co[0, 0]) and np.isfinite(co[1:]).all()
                    km = KMeans3f(x).cluster(c0.copy(), max_iter=iters, tol=0.0, use_kd_tree=kd)
                    sh = HipKMeansShard(x, k)
                    sk = ShardedKMeans3f(sh).cluster(c0.copy(), max_iter=iters, tol=0.0, use_kd_tree=kd)
                    sh.close()
                    report["cases"] += 1
                    for pname, got in (("cilhip_kmeans3f", km), ("shard loop", sk)):
                        gc, gl = got.getClusterCentroids(), got.getPointToClusterIndexMap()
                        tag = (n, shift, k, "kd" if kd else "brute", iters, pname)
                        if got.getNumberOfPerformedIterations() != ito:
                            failures.append(tag + ("iterations", got.getNumberOfPerformedIterations(), ito))
                        if not np.array_equal(np.isnan(gc), np.isnan(co)):
                            failures.append(tag + ("NaN pattern", np.argwhere(np.isnan(gc) != np.isnan(co))[:4].tolist(), gc[0].tolist(), co[0].tolist()))
                            continue
                        m = ~np.isnan(co)
                        if not np.array_equal(gc.view(np.uint32)[m], co.view(np.uint32)[m]):
                            failures.append(tag + ("centroids", int(np.count_nonzero(gc.view(np.uint32)[m] != co.view(np.uint32)[m])), gc[0].tolist(), co[0].tolist()))
                        if not np.array_equal(gl, lo):
                            failures.append(tag + ("labels", int(np.count_nonzero(gl != lo))))
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_kmeans_non_finite.json", report)
    assert not failures, failures[:6]


# --------------------------------------------------------------------------------------------------------------------------------
# plane RANSAC
# --------------------------------------------------------------------------------------------------------------------------------

PLANE_MS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257)
PLANE_NS = (2047, 2048, 2049, 262_143, 262_145, 2_097_151, 2_097_153, 2_099_201, 4_196_353)
TRUE_PLANE = np.array([0.3, -0.2, -1.0, 0.1]) / np.linalg.norm([0.3, -0.2, -1.0])


@pytest.fixture(scope="module")
def plane_cloud():
    return _plane_cloud(PLANE_NS[-1], 23)[0]


def _planes(m, rng):
    """m planes with clearly different inlier counts: every fourth is the cloud's own plane pushed away step by step (60 % of the
    points down to none), the others cut the cube at random; one NaN plane in the middle of every round of 64"""
    p = rng.standard_normal((m, 4))
    p[:, :3] /= np.linalg.norm(p[:, :3], axis=1, keepdims=True)
    p[:, 3] *= 0.3
    for j in range(0, m, 4):
        p[j] = TRUE_PLANE
        p[j, 3] += 0.0015 * (j // 4)
    p = p.astype(np.float32)
    for j in range(31, m, 64):
        p[j] = [0.0, np.nan, 0.0, 0.0]
    return p


def test_plane_counts_per_hypothesis_past_the_first_trip(orc, hip_lib, plane_cloud):
    """countInliers of 1..257 planes, exact per plane, at n around one tile (2048), around the first carried chunk of the final
    pass (262 144) and past the first grid trip of the scoring kernel (1024 blocks x 2048 points = 2 097 152; 2 099 201 = one
    more tile and a point; 4 196 353 = a third trip).  A count that lands in a neighbouring lane, round or tile shows."""
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    rng = np.random.default_rng(29)
    planes = _planes(257, rng)
    thr = 0.02
    failures = []
    report = {"cases": 0}
    t0 = time.time()
    for n in PLANE_NS:
        x = np.ascontiguousarray(plane_cloud[:n])
        want = np.array([orc.plane_count_inliers_mt(x, p, thr) for p in planes])
        assert want[31] == 0 and want[0] > 0.5 * n
        report[f"n={n}/distinct counts among 257"] = int(len(np.unique(want)))
        pe = PlaneRANSACEstimator3f(x)
        for m in PLANE_MS:
            # (the planes of a call start at another place of the set each time, so that lane h does not always hold the same plane)
            for first in (0, 257 - m):
                got = pe.countInliers(planes[first:first + m], thr)
                report["cases"] += 1
                if not np.array_equal(got, want[first:first + m]):
                    w = np.nonzero(got != want[first:first + m])[0]
                    failures.append((n, m, first, len(w), w[:6].tolist(), got[w[:6]].tolist(), want[first:first + m][w[:6]].tolist()))
    report["seconds"] = round(time.time() - t0, 1)
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_plane_counts.json", report)
    assert not failures, failures[:6]


def _check_plane_run(orc, x, thr, samples, max_iter, target, re_est, tag, failures, mean_abs=0.0):
    """one whole run with explicit samples against the oracle's: iteration count, winner, the residuals of the product's own
    model bit for bit, the inlier list element for element"""
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    pe = (PlaneRANSACEstimator3f(x).setMaxInlierResidual(thr).setTargetInlierCount(target).setMaxNumberOfIterations(max_iter)
          .setReEstimationStep(re_est).setSamples(samples))
    pl = pe.estimate().getModel()
    plo, reso, inlo, ito = orc.plane_ransac(x, samples, thr, target, max_iter=max_iter, re_estimate=re_est, mode=1)
    if pe.getNumberOfPerformedIterations() != ito:
        failures.append(tag + ("iterations", pe.getNumberOfPerformedIterations(), ito))
    if np.isnan(plo).any() or np.isnan(pl).any():
        if not np.array_equal(np.isnan(pl), np.isnan(plo)):
            failures.append(tag + ("NaN model", pl.tolist(), plo.tolist()))
    else:
        s = 1.0 if np.dot(pl[:3], plo[:3]) > 0 else -1.0
        dn = float(np.abs(pl[:3] - s * plo[:3]).max())
        do = float(abs(pl[3] - s * plo[3]))
        if dn > 2e-6 or do > 2e-6 * (1.0 + mean_abs):
            failures.append(tag + ("model", dn, do, pl.tolist(), plo.tolist()))
    res = pe.getModelResiduals()
    inl = pe.getModelInliers()
    if len(x) and not np.isnan(pl).any():
        chk = orc.plane_residuals(x, pl)
        if not np.array_equal(res.view(np.uint32), chk.view(np.uint32)):
            failures.append(tag + ("residuals", int(np.count_nonzero(res.view(np.uint32) != chk.view(np.uint32)))))
        want = np.nonzero(chk <= np.float32(thr))[0]
        if not np.array_equal(inl, want):
            failures.append(tag + ("inlier list", len(inl), len(want), int(np.count_nonzero(inl[:min(len(inl), len(want))] != want[:min(len(inl), len(want))]))))
        if len(np.setxor1d(want, inlo)) > max(3, int(2e-5 * len(x))):
            failures.append(tag + ("inliers against the oracle's run", len(want), len(inlo)))
        if pe.targetInlierCountAchieved() != (len(want) >= min(target, len(x))):
            failures.append(tag + ("target flag",))
    return pe, (plo, inlo, ito)


def test_plane_runs_past_the_first_chunk_and_trip(orc, hip_lib, plane_cloud):
    """Whole runs at n = 262 145 (the final pass carries its running offset from chunk to chunk) and 2 099 201 (a second tile per
    block in the scoring kernel): max_iter 1, 127, 129 (a partial round, one hypothesis into the second round), with and without
    re-estimation; a target the loop never reaches (all iterations run) and one it reaches early."""
    rng = np.random.default_rng(37)
    failures = []
    report = {"runs": 0}
    thr = 0.01
    for n in (262_145, 2_099_201):
        x = np.ascontiguousarray(plane_cloud[:n])
        for max_iter in (1, 127, 129):
            samples = rng.integers(0, n, (max_iter, 3)).astype(np.uint32)
            for re_est in (True, False):
                for target in (n, int(0.55 * n)):
                    pe, (plo, inlo, ito) = _check_plane_run(orc, x, thr, samples, max_iter, target, re_est, (n, max_iter, re_est, target), failures)
                    report["runs"] += 1
                    report[f"n={n}/max_iter={max_iter}/re={int(re_est)}/target={target}"] = {"iterations": ito, "inliers": int(pe.getNumberOfInliers())}
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_plane_runs.json", report)
    assert not failures, failures[:6]


def test_plane_ransac_in_other_frames(orc, hip_lib, plane_cloud):
    """The plane cloud (262 145 points) at (1e3, -250, 37): counts exact, the run against the oracle's with the normal within 2e-6
    and the offset within 2e-6 (1 + sum |mean_i|) (it is -n.mean in f32: the normal's last bits times the centroid).  Times 2^12
    and 2^-12 with the threshold and the planes' offsets scaled alike: counts, iteration count and inlier list identical to the
    unscaled run's; the normal bit for bit, or within 1e-6 and recorded where the f64 eigen-solve is not exactly equivariant."""
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    rng = np.random.default_rng(43)
    n = 262_145
    base = np.ascontiguousarray(plane_cloud[:n])
    thr = 0.01
    planes = _planes(129, rng)
    samples = rng.integers(0, n, (129, 3)).astype(np.uint32)
    failures = []
    report = {}
    unit = {}
    for name, scale, off in (("identity", 1.0, (0.0, 0.0, 0.0)), ("at (1e3, -250, 37)", 1.0, (1e3, -250.0, 37.0)), ("x 2^12", 2.0 ** 12, (0.0, 0.0, 0.0)),
                             ("x 2^-12", 2.0 ** -12, (0.0, 0.0, 0.0))):
        x = _mv(base, scale, off)
        pl = planes.astype(np.float64)
        pl[:, 3] = pl[:, 3] * scale - pl[:, :3] @ np.asarray(off)
        pl = pl.astype(np.float32)
        t = np.float32(thr * scale)
        got = PlaneRANSACEstimator3f(x).countInliers(pl, float(t))
        want = np.array([orc.plane_count_inliers_mt(x, p, float(t)) for p in pl])
        if not np.array_equal(got, want):
            failures.append((name, "counts", int(np.count_nonzero(got != want))))
        mean_abs = float(np.abs(x.astype(np.float64).mean(axis=0)).sum())
        runs = {}
        for re_est in (True, False):
            pe, (plo, inlo, ito) = _check_plane_run(orc, x, float(t), samples, 129, n, re_est, (name, re_est), failures, mean_abs)
            runs[re_est] = (pe.getModel().copy(), pe.getModelInliers().copy(), pe.getNumberOfPerformedIterations())
        if name == "identity":
            unit = {"counts": got, "runs": runs}
        elif name.startswith("x 2^"):
            if not np.array_equal(got, unit["counts"]):
                failures.append((name, "counts are not the unscaled cloud's", int(np.count_nonzero(got != unit["counts"]))))
            for re_est in (True, False):
                (m1, i1, it1), (m0, i0, it0) = runs[re_est], unit["runs"][re_est]
                if it1 != it0 or not np.array_equal(i1, i0):
                    failures.append((name, re_est, "iterations / inlier list are not the unscaled run's", it1, it0, len(i1), len(i0)))
                want_m = m0.copy(); want_m[3] = np.float32(float(m0[3]) * scale)
                if not np.array_equal(m1.view(np.uint32), want_m.view(np.uint32)):
                    dn = float(np.abs(m1[:3].astype(np.float64) - m0[:3]).max())
                    do = float(abs(float(m1[3]) / scale - float(m0[3])))
                    report[f"{name}/re={int(re_est)}/model not bitwise"] = {"normal": dn, "offset (unscaled)": do}
                    if dn > 1e-6 or do > 1e-6:
                        failures.append((name, re_est, "model", dn, do))
        report[name] = {"inliers": {int(k): int(len(v[1])) for k, v in runs.items()}}
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_plane_frames.json", report)
    assert not failures, failures[:6]


def test_plane_ransac_on_clouds_of_0_to_3_points(orc, hip_lib, plane_cloud):
    """0, 1, 2, 3 points, max_iter 4, explicit samples: model (NaN positions equal), inlier list and iteration count the oracle's"""
    from cilantro_amd.model_estimation import PlaneRANSACEstimator3f

    rng = np.random.default_rng(47)
    failures = []
    report = {}
    for npts in (0, 1, 2, 3):
        x = np.ascontiguousarray(plane_cloud[:npts])
        samples = rng.integers(0, max(npts, 1), (4, 3)).astype(np.uint32)
        if npts == 3:
            samples[0] = [0, 1, 2]
        for re_est in (True, False):
            pe = (PlaneRANSACEstimator3f(x).setMaxInlierResidual(0.01).setMaxNumberOfIterations(4).setReEstimationStep(re_est).setSamples(samples))
            pl = pe.estimate().getModel()
            plo, reso, inlo, ito = orc.plane_ransac(x, samples, 0.01, npts // 2 + npts % 2, max_iter=4, re_estimate=re_est, mode=1)
            report[f"{npts} points/re={int(re_est)}"] = {"iterations": [pe.getNumberOfPerformedIterations(), ito], "model": [pl.tolist(), plo.tolist()],
                                                        "inliers": [pe.getModelInliers().tolist(), inlo.tolist()]}
            if pe.getNumberOfPerformedIterations() != ito:
                failures.append((npts, re_est, "iterations", pe.getNumberOfPerformedIterations(), ito))
            if not np.array_equal(np.isnan(pl), np.isnan(plo)):
                failures.append((npts, re_est, "NaN model", pl.tolist(), plo.tolist()))
            elif not np.isnan(plo).any():
                s = 1.0 if np.dot(pl[:3], plo[:3]) > 0 else -1.0
                if np.abs(pl - s * plo).max() > 2e-6:
                    failures.append((npts, re_est, "model", pl.tolist(), plo.tolist()))
            if not np.array_equal(pe.getModelInliers(), inlo):
                failures.append((npts, re_est, "inliers", pe.getModelInliers().tolist(), inlo.tolist()))
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_plane_tiny.json", report)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------------------------
# rigid-transform RANSAC
# --------------------------------------------------------------------------------------------------------------------------------

TRANSFORM_MS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129)
TRANSFORM_NS = (1023, 1024, 1025, 131_071, 131_073, 1_048_575, 1_048_577, 1_049_601, 2_098_177)


@pytest.fixture(scope="module")
def pair_cloud():
    from cilantro_amd import synthetic as syn

    rng = np.random.default_rng(53)
    n = TRANSFORM_NS[-1]
    src = rng.random((n, 3)).astype(np.float32)
    T = np.eye(4); T[:3, :3] = syn.rot_xyz(0.25, -0.4, 0.1); T[:3, 3] = [0.2, 0.1, -0.3]
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3] + rng.normal(0, 5e-4, (n, 3))).astype(np.float32)
    bad = rng.random(n) < 0.45
    dst[bad] = (rng.random((int(bad.sum()), 3)) * 2.0 - 0.5).astype(np.float32)
    return dst, src, T


def _transforms(m, T, rng):
    """every fourth: the true motion pushed away step by step (clearly different counts); the others random; a NaN one per round"""
    from cilantro_amd import synthetic as syn

    Ts = np.tile(np.eye(4, dtype=np.float32), (m, 1, 1))
    for j in range(m):
        if j % 4 == 0:
            Ts[j] = T.astype(np.float32)
            Ts[j, 0, 3] += np.float32(0.0002 * (j // 4))
        else:
            Ts[j, :3, :3] = syn.rot_xyz(*(rng.normal(0, 0.3, 3))).astype(np.float32)
            Ts[j, :3, 3] = rng.normal(0, 0.2, 3).astype(np.float32)
    for j in range(31, m, 64):
        Ts[j, 1, 1] = np.nan
    return Ts


def test_transform_counts_and_runs_past_the_first_trip(orc, hip_lib, pair_cloud):
    """The plane tests' twins: countInliers of 1..129 transforms exact per transform at n around a tile (1024), around the first
    chunk carry (131 072) and past the first grid trip (1 048 576); whole runs at n = 1 050 001 with max_iter 1, 127, 129, with
    and without re-estimation -- iteration count and winner the oracle's, residuals of the product's own model bit for bit, the
    inlier list element for element."""
    from cilantro_amd.model_estimation import RigidTransformRANSACEstimator3f

    dst_all, src_all, T = pair_cloud
    rng = np.random.default_rng(59)
    Ts = _transforms(129, T, rng)
    thr = 2e-3
    failures = []
    report = {"count cases": 0, "runs": 0}
    for n in TRANSFORM_NS:
        dst, src = np.ascontiguousarray(dst_all[:n]), np.ascontiguousarray(src_all[:n])
        want = np.array([orc.transform_count_inliers(dst, src, t, thr) for t in Ts])
        assert want[31] == 0 and want[0] > 0.4 * n
        report[f"n={n}/distinct counts among 129"] = int(len(np.unique(want)))
        te = RigidTransformRANSACEstimator3f(dst, src)
        for m in TRANSFORM_MS:
            for first in (0, 129 - m):
                got = te.countInliers(Ts[first:first + m], thr)
                report["count cases"] += 1
                if not np.array_equal(got, want[first:first + m]):
                    w = np.nonzero(got != want[first:first + m])[0]
                    failures.append((n, m, first, len(w), w[:6].tolist(), got[w[:6]].tolist(), want[first:first + m][w[:6]].tolist()))
    n = 1_050_001
    dst, src = np.ascontiguousarray(dst_all[:n]), np.ascontiguousarray(src_all[:n])
    for max_iter in (1, 127, 129):
        samples = rng.integers(0, n, (max_iter, 3)).astype(np.uint32)
        for re_est in (True, False):
            for target in (n, int(0.5 * n)):
                tag = (n, max_iter, re_est, target)
                te = (RigidTransformRANSACEstimator3f(dst, src).setMaxInlierResidual(thr).setTargetInlierCount(target)
                      .setMaxNumberOfIterations(max_iter).setReEstimationStep(re_est).setSamples(samples))
                Tg = te.estimate().getModel()
                To, reso, inlo, ito, haveo = orc.transform_ransac(dst, src, samples, thr, target, max_iter=max_iter, re_estimate=re_est, mode=orc.MODE_MIXED)
                report["runs"] += 1
                if te.getNumberOfPerformedIterations() != ito:
                    failures.append(tag + ("iterations", te.getNumberOfPerformedIterations(), ito))
                if np.abs(Tg - To).max() > 5e-6:
                    failures.append(tag + ("transform", float(np.abs(Tg - To).max())))
                res = te.getModelResiduals()
                if len(res) == 0 and len(inlo) == 0:
                    continue      # (no accepted hypothesis and no re-estimation: the reference's residuals stay empty)
                chk = orc.transform_residuals(dst, src, Tg)
                if not np.array_equal(res.view(np.uint32), chk.view(np.uint32)):
                    failures.append(tag + ("residuals", len(res), int(np.count_nonzero(res.view(np.uint32) != chk.view(np.uint32))) if len(res) == len(chk) else -1))
                want_i = np.nonzero(chk <= np.float32(thr))[0]
                if not np.array_equal(te.getModelInliers(), want_i):
                    failures.append(tag + ("inlier list", len(te.getModelInliers()), len(want_i)))
                if len(np.setxor1d(want_i, inlo)) > max(3, int(2e-4 * n)):
                    failures.append(tag + ("inliers against the oracle's run", len(want_i), len(inlo)))
    # 0-3 pairs, max_iter 4: iteration count and inlier list the oracle's (the motion through one or two pairs is not unique)
    for npts in (0, 1, 2, 3):
        samples = rng.integers(0, max(npts, 1), (4, 3)).astype(np.uint32)
        if npts == 3:
            samples[:] = [0, 1, 2]
        for re_est in (True, False):
            te = (RigidTransformRANSACEstimator3f(dst_all[:npts].copy(), src_all[:npts].copy()).setMaxInlierResidual(thr).setMaxNumberOfIterations(4)
                  .setReEstimationStep(re_est).setSamples(samples).estimate())
            To, reso, inlo, ito, haveo = orc.transform_ransac(dst_all[:npts].copy(), src_all[:npts].copy(), samples, thr, npts // 2 + npts % 2, max_iter=4,
                                                              re_estimate=re_est, mode=orc.MODE_MIXED)
            report[f"{npts} pairs/re={int(re_est)}"] = {"iterations": [te.getNumberOfPerformedIterations(), ito], "inliers": [te.getModelInliers().tolist(), inlo.tolist()]}
            if te.getNumberOfPerformedIterations() != ito or not np.array_equal(te.getModelInliers(), inlo):
                failures.append((npts, re_est, "tiny", te.getNumberOfPerformedIterations(), ito, te.getModelInliers().tolist(), inlo.tolist()))
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_transform.json", report)
    assert not failures, failures[:6]


# --------------------------------------------------------------------------------------------------------------------------------
# radius lists, normals and limits off the origin
# --------------------------------------------------------------------------------------------------------------------------------

LIST_FRAMES = (("at (1e3, -250, 37)", (1e3, -250.0, 37.0)), ("at 4096", 4096.0))


def test_radius_lists_off_the_origin(orc, hip_lib):
    """radiusSearch lists -- offsets, indices, d2 bits -- on the cloud of test_radius_search_lists_vs_oracle moved to
    (1e3, -250, 37) and to 4096 (coordinates quantised to 2^-11: many exactly equal distances, the order is (distance, index)),
    for 1, 63, 65 and 257 queries."""
    from cilantro_amd.normal_estimation import KDTree3f

    rng = np.random.default_rng(17)
    pts0 = rng.random((30_000, 3)).astype(np.float32)
    pts0[100:110] = pts0[100]
    q0 = np.concatenate([pts0[:150], rng.random((107, 3)).astype(np.float32) * 1.3 - 0.15]).astype(np.float32)
    report = {}
    failures = []
    for name, off in LIST_FRAMES:
        pts, q = _mv(pts0, 1.0, off), _mv(q0, 1.0, off)
        tree = KDTree3f(pts)
        for nq in (1, 63, 65, 257):
            for r2 in (0.02 ** 2, 0.09 ** 2):
                goff, gidx, gd2 = tree.radiusSearch(q[:nq], r2)
                ooff, oidx, od2 = orc.radius_search(pts, q[:nq], r2)
                same = (np.array_equal(goff, ooff) and np.array_equal(gidx, oidx) and np.array_equal(gd2.view(np.uint32), od2.view(np.uint32)))
                if nq == 257:
                    tied = sum(int(len(od2[a:b]) - len(np.unique(od2[a:b]))) for a, b in zip(ooff[:-1], ooff[1:]))
                    report[f"{name}/r2={r2:.4g}"] = {"neighbours": int(len(oidx)), "equal distances inside a list": tied}
                if not same:
                    failures.append((name, nq, r2, len(gidx), len(oidx)))
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_radius_lists.json", report)
    assert not failures, failures


def test_normals_off_the_origin(orc, hip_lib):
    """getNormalsAndCurvatureKNN / KNNInRadius / Radius on the sheet cloud of test_knn_and_normal_estimation_vs_oracle moved to
    (1e3, -250, 37) and to 4096, against the oracle (mode 1) with that test's criteria: NaN pattern equal, at least 99.9 % of the
    well-defined normals with dot > 1 - 1e-4, curvature within 1e-4, normals on the view point's side."""
    from cilantro_amd.normal_estimation import NormalEstimation3f

    rng = np.random.default_rng(11)
    n = 120_000
    x0 = rng.random((n, 3)).astype(np.float32)
    m = n // 2
    x0[:m, 2] = (0.2 * x0[:m, 0] + 0.1 * np.sin(6 * x0[:m, 1]) + rng.normal(0, 1e-3, m)).astype(np.float32)
    report = {}
    failures = []
    for name, off in LIST_FRAMES:
        x = _mv(x0, 1.0, off)
        o3 = np.broadcast_to(np.asarray(off, np.float64), (3,))
        rad = np.float32(0.012)
        for cname, k, r2, vp0 in (("knn 10", 10, np.inf, [0.5, 0.5, 10.0]), ("knn 7, no view point", 7, np.inf, None),
                                  ("knn 12 in radius", 12, np.float32(0.015) ** 2, [0.0, 0.0, -5.0]), ("radius", None, rad * rad, [0.5, 0.5, 10.0])):
            vp = None if vp0 is None else (np.asarray(vp0, np.float64) + o3).astype(np.float32).tolist()
            ne = NormalEstimation3f(x).setViewPoint(vp)
            if k is None:
                ng, cg = ne.getNormalsAndCurvatureRadius(rad)
                no, co = orc.normals_radius(x, r2, vp, mode=1)
            else:
                ng, cg = (ne.getNormalsAndCurvatureKNN(k) if np.isinf(r2) else ne.getNormalsAndCurvatureKNNInRadius(k, np.sqrt(np.float32(r2))))
                no, co = orc.normals_knn(x, k, r2, vp, mode=1)
            nan_g, nan_o = np.isnan(ng).any(axis=1), np.isnan(no).any(axis=1)
            ok = ~(nan_g | nan_o)
            dots = (ng[ok] * no[ok]).sum(axis=1)
            if vp is None:
                dots = np.abs(dots)
            well = cg[ok] < 0.2
            share = float((dots[well] > 1 - 1e-4).mean())
            cerr = float(np.nanmax(np.abs(cg[ok] - co[ok])))
            side = True if vp is None else bool((((np.asarray(vp, np.float32) - x[ok]) * ng[ok]).sum(axis=1) >= -1e-6).all())
            report[f"{name}/{cname}"] = {"NaN rows": [int(nan_g.sum()), int(nan_o.sum())], "share of well-defined normals with dot > 1 - 1e-4": share,
                                         "largest curvature difference": cerr, "view point side": side}
            if not np.array_equal(nan_g, nan_o):
                failures.append((name, cname, "NaN pattern", int(np.count_nonzero(nan_g != nan_o))))
            if not share > 0.999:
                failures.append((name, cname, "share", share))
            if not cerr < 1e-4:
                failures.append((name, cname, "curvature", cerr))
            if not side:
                failures.append((name, cname, "view point side"))
            if k is None and not 0 < nan_g.sum() < n:
                failures.append((name, cname, "no sparse region"))
    report["failures"] = [str(f) for f in failures]
    _report("model_kernels_normals_frames.json", report)
    assert not failures, failures


def test_knn_list_length_limit(orc, hip_lib):
    """k = 32 (the longest list) equals the oracle's slot for slot; k = 33 is the documented invalid-argument code from kNNSearch
    and from the normal estimator"""
    from cilantro_amd.normal_estimation import KDTree3f, NormalEstimation3f

    rng = np.random.default_rng(67)
    report = {}
    for name, off in (("origin", 0.0),) + LIST_FRAMES:
        x = _mv(rng.random((50_000, 3)).astype(np.float32), 1.0, off)
        q = _mv(rng.random((3001, 3)).astype(np.float32), 1.0, off)
        gi, gd, gc = KDTree3f(x).kNNSearch(q, 32)
        oi, od, oc = orc.knn_batch(orc.KDTree(x), q, 32)
        assert np.array_equal(gc, oc) and (gc == 32).all(), name
        assert np.array_equal(gd.view(np.uint32), od.view(np.uint32)), name
        assert np.array_equal(gi, oi), (name, np.nonzero((gi != oi).any(axis=1))[0][:5])
        with pytest.raises(capi.CilhipError) as e:
            KDTree3f(x).kNNSearch(q, 33)
        assert e.value.code == capi.ERR_INVALID
        with pytest.raises(capi.CilhipError) as e:
            NormalEstimation3f(x).getNormalsAndCurvatureKNN(33)
        assert e.value.code == capi.ERR_INVALID
        report[name] = {"queries": int(len(q)), "k = 32 rows differing": int(np.count_nonzero((gi != oi).any(axis=1))), "k = 33": "invalid argument"}
    _report("model_kernels_knn_limit.json", report)
