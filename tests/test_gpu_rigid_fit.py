"""GPU: the closed-form rigid fit (kabsch_from_sums, csrc/solve.hpp) on the device, through every public path that reaches it, on the
inputs where it leaves the polar iteration for the SVD and the reflection fix: one, two and three pairs (three pairs are coplanar about
their centroid: every RANSAC hypothesis is a fallback fit), repeated, identical and collinear samples, mirrored and coplanar sets --
as they are, off the origin and rescaled.  The yardstick is optimality (tests/_rigid_refs.py, pinned on the CPU by
tests/test_rigid_refs_cpu.py): the returned motion is finite, a proper rotation to 4 u, and costs no more than the optimum plus the
derived bound.  Where the model is unique -- samples, scores, residuals, inlier lists -- the comparisons are exact.  Every test prints
its figures and writes them as rigid_fit_*.json (_report)."""
import ctypes as C

import numpy as np
import pytest

import _rigid_refs as R
from cilantro_amd import capi
from test_gpu_model_kernels import _transforms, pair_cloud  # noqa: F401  (the fixture of the existing transform tests)
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
N_FRAMES = 131_073
THR = 2e-3


def _est(dst, src):
    from cilantro_amd.model_estimation import RigidTransformRANSACEstimator3f

    return RigidTransformRANSACEstimator3f(np.ascontiguousarray(dst, F32), np.ascontiguousarray(src, F32))


def _fit_device(dst, src):
    """cilhip_transform_fit3f with CILHIP_MEM_DEVICE input"""
    import torch

    n = len(dst)
    d, s = torch.from_numpy(np.ascontiguousarray(dst, F32)).cuda(), torch.from_numpy(np.ascontiguousarray(src, F32)).cuda()
    torch.cuda.synchronize()
    T = np.full(16, 7.0, F32)
    rc = capi.load().cilhip_transform_fit3f(0, d.data_ptr() if n else None, s.data_ptr() if n else None, n, capi.MEM_DEVICE, T.ctypes.data)
    assert rc == capi.OK, rc
    return T.reshape(4, 4).T.copy()


def _short(f):
    return {"excess": f["excess"], "bound": f["bound"], "scale": f["scale"]}


# ---- 1. estimateModel over all pairs --------------------------------------------------------------------------------------------
def test_fit_over_all_pairs_on_the_case_table(hip_lib):
    report = {}
    for fi, (fname, _, _) in enumerate(R.FRAMES):
        for name, d, s in R.cases(fi):
            Th = _est(d, s).estimateModel()
            Td = _fit_device(d, s)
            report[f"{fname}/{name}"] = _short(R.check(Th, d, s, f"{fname}/{name}"))
            assert Th.tobytes() == Td.tobytes(), (fname, name, Th.tolist(), Td.tolist())
    _report("rigid_fit_table.json", report)


FIT_SIZES = (1, 2, 3, 4, 255, 256, 257, 262_143, 262_145)


@pytest.mark.parametrize("kind", ["generic", "mirrored", "coplanar"])
def test_fit_over_all_pairs_at_block_and_trip_edges(hip_lib, kind):
    """one block of 256 lanes +- 1; 1024 blocks x 256 lanes +- 1 (the grid-stride loop of k_tmoments takes a second trip)"""
    D, S = R.family(kind, FIT_SIZES[-1])
    report = {}
    for n in FIT_SIZES:
        d, s = D[:n], S[:n]
        Th = _est(d, s).estimateModel()
        report[f"n={n}"] = _short(R.check(Th, d, s, f"{kind}/n={n}"))
        assert Th.tobytes() == _fit_device(d, s).tobytes(), (kind, n)
    _report(f"rigid_fit_sizes_{kind}.json", report)


def test_fit_of_no_pairs_is_the_identity(hip_lib):
    e = np.zeros((0, 3), F32)
    eye = np.eye(4, dtype=F32)
    assert _est(e, e).estimateModel().tobytes() == eye.tobytes()
    assert _fit_device(e, e).tobytes() == eye.tobytes()


# ---- 2. one hypothesis at a time ------------------------------------------------------------------------------------------------
def _one_hypothesis(dst, src, samples, max_iter, target=None):
    te = _est(dst, src).setMaxInlierResidual(float("inf")).setMaxNumberOfIterations(max_iter).setReEstimationStep(False).setSamples(samples)
    if target is not None:
        te.setTargetInlierCount(target)
    return te.estimate()


def test_one_hypothesis_from_a_degenerate_sample(hip_lib):
    """k_tmodels: the sample is pairs 0, 1, 2 of a cloud of 1025 pairs (the scoring kernel has a tail), infinite threshold, no
    re-estimation: the model is the fit of exactly those three pairs.  Then the same sample as hypothesis 63 (the last lane of the first
    round), 64 and 65 (the second round) behind hypotheses that all name pair 1025, whose src row holds a NaN: each of those is counted
    and never accepted, and the model's bytes are those of the single-hypothesis run."""
    report = {}
    for fi, (fname, scale, off) in enumerate(R.FRAMES):
        filler_s = np.random.default_rng(300).random((1022, 3))
        filler_d = np.random.default_rng(301).random((1022, 3))
        for name, d3, s3 in R.cases(fi):
            if name not in R.THREE_PAIR:
                continue
            dst = np.concatenate([d3, R.in_frame(filler_d, scale, off)])
            src = np.concatenate([s3, R.in_frame(filler_s, scale, off)])
            assert len(dst) == 1025
            te = _one_hypothesis(dst, src, np.array([[0, 1, 2]], np.uint32), 1)
            T1 = te.getModel()
            report[f"{fname}/{name}"] = _short(R.check(T1, d3, s3, f"{fname}/{name}"))
            assert te._raw.have_model == 1 and te.getNumberOfPerformedIterations() == 1
            assert np.array_equal(te.getModelInliers(), np.arange(1025)), (fname, name, len(te.getModelInliers()))
            # the same cloud and one more pair with a NaN in its src row
            dst2 = np.concatenate([dst, dst[5:6]])
            src2 = np.concatenate([src, src[5:6]])
            src2[1025, 1] = np.nan
            for pos in (63, 64, 65):
                samples = np.tile(np.array([[1025, 3, 4]], np.uint32), (66, 1))
                samples[pos] = [0, 1, 2]
                te2 = _one_hypothesis(dst2, src2, samples, 66, target=1025)
                assert te2.getNumberOfPerformedIterations() == pos + 1, (fname, name, pos, te2.getNumberOfPerformedIterations())
                assert te2.getModel().tobytes() == T1.tobytes(), (fname, name, pos, te2.getModel().tolist(), T1.tolist())
                assert te2._raw.have_model == 1 and np.array_equal(te2.getModelInliers(), np.arange(1025))
    _report("rigid_fit_hypotheses.json", report)


# ---- 3. re-estimation over a degenerate inlier set ------------------------------------------------------------------------------
def _own_residuals_and_inliers(orc, te, dst, src, thr, tag):
    T = te.getModel()
    res = te.getModelResiduals()
    chk = orc.transform_residuals(dst, src, T)
    assert np.array_equal(res.view(np.uint32), chk.view(np.uint32)), (tag, "residuals", int(np.count_nonzero(res.view(np.uint32) != chk.view(np.uint32))))
    want = np.nonzero(chk <= F32(thr))[0]
    assert np.array_equal(te.getModelInliers(), want), (tag, "inlier list", len(te.getModelInliers()), len(want))
    return want


@pytest.mark.parametrize("kind", ["coplanar", "mirrored"])
def test_re_estimation_over_a_degenerate_inlier_set(orc, hip_lib, kind):
    """4097 pairs, 60 % of them inliers of the base motion: all on one plane, or mirrored in z (the sample's three pairs then define a
    proper rotation that only a thin slab of the mirrored pairs follows: a nearly flat set whose best orthogonal fit is a reflection).
    Run A, without re-estimation: residuals and inlier list I0 exact for its own model.  Run B, with it: the model is the optimal fit
    of the pairs I0, and its own residuals and inlier list are exact again."""
    n = 4097
    rng = np.random.default_rng(400)
    src = rng.random((n, 3))
    inl = np.sort(rng.permutation(n)[: int(0.6 * n)])
    if kind == "coplanar":
        src[inl, 2] = 0.5
    dst = rng.random((n, 3)) * 2.0 - 0.5
    dst[inl] = (src[inl] @ R.MIRROR_Z if kind == "mirrored" else src[inl]) @ R.BASE_R.T + R.BASE_T
    dst, src = R.in_frame(dst, 1.0, 0.0), R.in_frame(src, 1.0, 0.0)
    thr = 1e-3 if kind == "coplanar" else 2e-2
    samples = inl[[10, 700, 1900]].astype(np.uint32).reshape(1, 3)
    runs = {}
    for re_est in (False, True):
        te = (_est(dst, src).setMaxInlierResidual(thr).setTargetInlierCount(n).setMaxNumberOfIterations(1).setReEstimationStep(re_est).setSamples(samples).estimate())
        assert te.getNumberOfPerformedIterations() == 1
        runs[re_est] = (te, _own_residuals_and_inliers(orc, te, dst, src, thr, (kind, re_est)))
    i0 = runs[False][1]
    assert len(i0) >= 3 and np.isin(i0, inl).all(), (kind, len(i0))
    if kind == "coplanar":
        assert np.array_equal(i0, inl)
    f = R.check(runs[True][0].getModel(), dst[i0], src[i0], f"{kind}/re-estimated over {len(i0)} pairs")
    _report(f"rigid_fit_re_estimation_{kind}.json", {"inliers of the sample's model": int(len(i0)), "inliers of the re-estimated model": int(len(runs[True][1])), **_short(f)})


# ---- 4. 0-3 pairs: the model too ------------------------------------------------------------------------------------------------
def test_runs_on_0_to_3_pairs_return_the_fit_of_the_sample(orc, hip_lib):
    """the tiny-input loop of test_transform_counts_and_runs_past_the_first_trip with the model checked: the first sample names every
    pair, its fit reaches them all, the loop stops there; with and without re-estimation the model is the optimal fit of those pairs --
    the identity for none, exactly R = I and t = d - s rounded to f32 for one"""
    _, d3, s3 = R.cases(0)[0]
    report = {}
    for npts in (0, 1, 2, 3):
        d, s = d3[:npts].copy(), s3[:npts].copy()
        samples = np.random.default_rng(47).integers(0, max(npts, 1), (4, 3)).astype(np.uint32)
        samples[0] = np.arange(3) % max(npts, 1)
        for re_est in (True, False):
            te = _est(d, s).setMaxInlierResidual(THR).setMaxNumberOfIterations(4).setReEstimationStep(re_est).setSamples(samples).estimate()
            To, reso, inlo, ito, haveo = orc.transform_ransac(d, s, samples, THR, npts // 2 + npts % 2, max_iter=4, re_estimate=re_est, mode=orc.MODE_MIXED)
            T = te.getModel()
            assert te.getNumberOfPerformedIterations() == ito == 1 and np.array_equal(te.getModelInliers(), inlo), (npts, re_est, ito, inlo.tolist())
            assert np.array_equal(te.getModelInliers(), np.arange(npts))
            report[f"{npts} pairs/re={int(re_est)}"] = _short(R.check(T, d, s, f"{npts} pairs/re={int(re_est)}"))
            if npts == 0:
                assert T.tobytes() == np.eye(4, dtype=F32).tobytes()
            if npts == 1:
                want = np.eye(4, dtype=F32)
                want[:3, 3] = (d[0].astype(F64) - s[0].astype(F64)).astype(F32)
                assert T.tobytes() == want.tobytes(), (T.tolist(), want.tolist())
    _report("rigid_fit_tiny.json", report)


# ---- 5. other frames ------------------------------------------------------------------------------------------------------------
def _to_frame(Ts, scale, off):
    """d = R s + t in the cloud's frame -> d' = R s' + (scale t + off - R off) with x' = scale x + off"""
    out = Ts.copy()
    off = np.asarray(off, F64)
    for j in range(len(Ts)):
        Rj = Ts[j, :3, :3].astype(F64)
        out[j, :3, 3] = (Ts[j, :3, 3].astype(F64) * scale + off - Rj @ off).astype(F32)
    return out


def _run(dst, src, thr, samples, target, re_est):
    return (_est(dst, src).setMaxInlierResidual(thr).setTargetInlierCount(target).setMaxNumberOfIterations(len(samples)).setReEstimationStep(re_est)
            .setSamples(samples).estimate())


def test_transform_ransac_in_other_frames(orc, hip_lib, pair_cloud):  # noqa: F811
    """The twin of test_plane_ransac_in_other_frames on 131 073 pairs of the transform tests' cloud: at (1e3, -250, 37) the counts of
    129 transforms are exact and whole runs of 129 explicit samples follow the oracle's -- iterations, winner, residuals of the
    product's own model bit for bit, inlier list element for element; the rotation block within the existing 5e-6 and the translation
    within 5e-6 (1 + sum |mean_i|), mean the source centroid (t = mean_d - R mean_s: the rotation's last bits times the centroid, the
    plane test's reason for its offset).  Times 2^12 and 2^-12 with the threshold and the translations scaled alike: counts, iteration
    count and inlier list identical to the unscaled run's, the rotation block bit for bit and the translation exactly scaled, or within
    1e-6 and recorded where the f64 solve is not exactly equivariant."""
    dst_all, src_all, T = pair_cloud
    n = N_FRAMES
    rng = np.random.default_rng(61)
    Ts0 = _transforms(129, T, rng)
    samples = rng.integers(0, n, (129, 3)).astype(np.uint32)
    failures = []
    report = {}
    unit = {}
    for name, scale, off in R.FRAMES:
        dst, src = R.in_frame(dst_all[:n], scale, off), R.in_frame(src_all[:n], scale, off)
        Ts = _to_frame(Ts0, scale, off)
        thr = float(F32(THR * scale))
        got = _est(dst, src).countInliers(Ts, thr)
        want = np.array([orc.transform_count_inliers(dst, src, t, thr) for t in Ts])
        if name == "as is":
            assert want[31] == 0 and want[0] > 0.4 * n
        if not np.array_equal(got, want):
            failures.append((name, "counts", int(np.count_nonzero(got != want))))
        mean_abs = float(np.abs(src.astype(F64).mean(axis=0)).sum())
        runs = {}
        for re_est in (True, False):
            tag = (name, re_est)
            te = _run(dst, src, thr, samples, n, re_est)
            Tg = te.getModel()
            To, reso, inlo, ito, haveo = orc.transform_ransac(dst, src, samples, thr, n, max_iter=129, re_estimate=re_est, mode=orc.MODE_MIXED)
            if te.getNumberOfPerformedIterations() != ito:
                failures.append(tag + ("iterations", te.getNumberOfPerformedIterations(), ito))
            dr = float(np.abs(Tg[:3, :3].astype(F64) - To[:3, :3]).max())
            dt = float(np.abs(Tg[:3, 3].astype(F64) - To[:3, 3]).max())
            report[f"{name}/re={int(re_est)}"] = {"rotation against the oracle": dr, "translation against the oracle": dt, "translation tolerance": 5e-6 * (1.0 + mean_abs)}
            if dr > 5e-6 or dt > 5e-6 * (1.0 + mean_abs) or not np.array_equal(Tg[3], np.array([0, 0, 0, 1], F32)):
                failures.append(tag + ("transform", dr, dt))
            res = te.getModelResiduals()
            chk = orc.transform_residuals(dst, src, Tg)
            if not np.array_equal(res.view(np.uint32), chk.view(np.uint32)):
                failures.append(tag + ("residuals", int(np.count_nonzero(res.view(np.uint32) != chk.view(np.uint32))) if len(res) == len(chk) else -1))
            want_i = np.nonzero(chk <= F32(thr))[0]
            if not np.array_equal(te.getModelInliers(), want_i):
                failures.append(tag + ("inlier list", len(te.getModelInliers()), len(want_i)))
            if len(np.setxor1d(want_i, inlo)) > max(3, int(2e-4 * n)):
                failures.append(tag + ("inliers against the oracle's run", len(want_i), len(inlo)))
            report[f"{name}/re={int(re_est)}"]["inliers"] = int(len(want_i))
            runs[re_est] = (Tg.copy(), te.getModelInliers().copy(), te.getNumberOfPerformedIterations())
        if name == "as is":
            unit = {"counts": got, "runs": runs}
        elif name.startswith("x 2^"):
            if not np.array_equal(got, unit["counts"]):
                failures.append((name, "counts are not the unscaled cloud's", int(np.count_nonzero(got != unit["counts"]))))
            for re_est in (True, False):
                (m1, i1, it1), (m0, i0, it0) = runs[re_est], unit["runs"][re_est]
                if it1 != it0 or not np.array_equal(i1, i0):
                    failures.append((name, re_est, "iterations / inlier list are not the unscaled run's", it1, it0, len(i1), len(i0)))
                want_m = m0.copy()
                want_m[:3, 3] = (m0[:3, 3].astype(F64) * scale).astype(F32)
                if m1.tobytes() != want_m.tobytes():
                    dr = float(np.abs(m1[:3, :3].astype(F64) - m0[:3, :3]).max())
                    dt = float(np.abs(m1[:3, 3].astype(F64) / scale - m0[:3, 3]).max())
                    report[f"{name}/re={int(re_est)}/model not bitwise"] = {"rotation": dr, "translation (unscaled)": dt}
                    if dr > 1e-6 or dt > 1e-6:
                        failures.append((name, re_est, "model", dr, dt))
    report["failures"] = [str(f) for f in failures]
    _report("rigid_fit_frames.json", report)
    assert not failures, failures[:6]


# ---- 6. non-finite pairs --------------------------------------------------------------------------------------------------------
def test_non_finite_pairs(orc, hip_lib, pair_cloud):  # noqa: F811
    """300 of 131 073 pairs carry a NaN, +inf or -inf in one coordinate of dst or src (row 0, row n - 1, rows 1023, 1024, 1025 among
    them).  Such a pair is never an inlier and a sample that names one is counted and never accepted: scores, winner, iteration
    count, inlier list and the re-estimated model are those of the cloud without these rows."""
    dst_all, src_all, T = pair_cloud
    n = N_FRAMES
    rng = np.random.default_rng(67)
    dst, src = dst_all[:n].copy(), src_all[:n].copy()
    must = np.array([0, n - 1, 1023, 1024, 1025])
    rest = np.setdiff1d(rng.permutation(n)[:400], must)[:295]
    bad = np.sort(np.concatenate([must, rest]))
    assert len(bad) == 300 and {0, n - 1, 1023, 1024, 1025} <= set(bad.tolist())
    vals = (np.nan, np.inf, -np.inf)
    for k, r in enumerate(bad):
        (dst if (k // 3) % 2 == 0 else src)[r, (k // 6) % 3] = vals[k % 3]
    good = np.ones(n, bool)
    good[bad] = False
    new_index = np.cumsum(good) - 1
    dst_c, src_c = np.ascontiguousarray(dst[good]), np.ascontiguousarray(src[good])
    report = {"bad rows": int(len(bad))}
    # scoring
    Ts = _transforms(129, T, rng)
    got = _est(dst, src).countInliers(Ts, THR)
    want = np.array([orc.transform_count_inliers(dst_c, src_c, t, THR) for t in Ts])
    assert want[0] > 0.4 * n and np.array_equal(got, want), np.nonzero(got != want)[0][:6]
    # runs: bad rows named by the samples at positions 0, 63 and 64
    good_rows = np.nonzero(good)[0]
    samples = good_rows[rng.integers(0, len(good_rows), (129, 3))].astype(np.uint32)
    samples_c = new_index[samples].astype(np.uint32)
    outlier = int(np.nonzero(np.linalg.norm(orc.transform_points(T, src_c) - dst_c, axis=1) > 0.3)[0][0])
    for pos, row in ((0, [0, samples[0, 1], samples[0, 2]]), (63, [samples[63, 0], n - 1, samples[63, 2]]), (64, [samples[64, 0], samples[64, 1], 1024])):
        samples[pos] = row
        samples_c[pos] = [outlier, outlier, outlier]      # (the clean run's stand-in: a translation that reaches fewer than three pairs)
    stand_in = np.eye(4, dtype=F32)
    stand_in[:3, 3] = (dst_c[outlier].astype(F64) - src_c[outlier].astype(F64)).astype(F32)
    assert orc.transform_count_inliers(dst_c, src_c, stand_in, THR) < 3
    for re_est in (False, True):
        te = _run(dst, src, THR, samples, n, re_est)
        tc = _run(dst_c, src_c, THR, samples_c, len(dst_c), re_est)
        assert te.getNumberOfPerformedIterations() == tc.getNumberOfPerformedIterations() == 129
        assert te.getModel().tobytes() == tc.getModel().tobytes(), (re_est, te.getModel().tolist(), tc.getModel().tolist())
        assert np.isfinite(te.getModel()).all()
        inl = te.getModelInliers()
        assert not np.isin(inl, bad).any() and np.array_equal(new_index[inl], tc.getModelInliers()), (re_est, len(inl), len(tc.getModelInliers()))
        res = te.getModelResiduals()
        assert not np.isfinite(res[bad]).any(), res[bad][np.isfinite(res[bad])][:5]
        chk = orc.transform_residuals(dst_c, src_c, te.getModel())
        assert np.array_equal(res[good].view(np.uint32), chk.view(np.uint32)) and np.array_equal(tc.getModelResiduals().view(np.uint32), chk.view(np.uint32))
        report[f"re={int(re_est)}"] = {"iterations": te.getNumberOfPerformedIterations(), "inliers": int(len(inl))}
    # the first hypothesis alone: counted, not accepted
    te = _run(dst, src, THR, samples[:1], n, False)
    assert te.getNumberOfPerformedIterations() == 1 and te._raw.have_model == 0 and len(te.getModelInliers()) == 0
    # estimateModel over all pairs: not a finite, plausible-looking motion
    for rows in (bad, bad[:1], bad[-1:]):
        d1, s1 = dst_all[:n].copy(), src_all[:n].copy()
        d1[rows], s1[rows] = dst[rows], src[rows]
        Tm = _est(d1, s1).estimateModel()
        print("estimateModel with", len(rows), "bad rows:", Tm.tolist())
        assert not np.isfinite(Tm).all()
    _report("rigid_fit_non_finite.json", report)


# ---- 7. point-to-point ICP on coplanar clouds -----------------------------------------------------------------------------------
def test_point_to_point_icp_on_coplanar_clouds(hip_lib):
    """a wall: 4097 points on z = 0.5, the source moved inside the plane; one iteration from the identity is the rigid fit of the
    matched pairs by the single-lane device epilogue, whose sigma is singular -- per-lane and LDS-tiled search"""
    from cilantro_amd.icp import SimplePointToPointMetricRigidICP3f

    rng = np.random.default_rng(500)
    n = 4097
    dst = np.zeros((n, 3))
    dst[:, :2] = rng.random((n, 2))
    dst[:, 2] = 0.5
    a = 0.01
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    src = R.in_frame((dst - [0.5, 0.5, 0.5]) @ Rz.T + [0.502, 0.499, 0.5], 1.0, 0.0)
    dst = R.in_frame(dst, 1.0, 0.0)
    assert (src[:, 2] == 0.5).all() and (dst[:, 2] == 0.5).all()
    out = {}
    report = {}
    for tiled in (0, 2):
        icp = SimplePointToPointMetricRigidICP3f(dst, src)
        icp._ctx.set_option("tiled", tiled)
        icp.correspondenceSearchEngine().setMaxDistance(0.02 * 0.02)
        eng = icp.correspondenceSearchEngine()
        i1, i2, _ = eng.findCorrespondences(np.eye(4, dtype=F32)).getCorrespondences()
        assert len(i1) > 0.9 * n
        T = icp.setMaxNumberOfIterations(1).estimate().getTransform()
        assert icp.getNumberOfPerformedIterations() == 1 and icp.last_ncorr_ == len(i1)
        report[f"tiled={tiled}"] = {"pairs": int(len(i1)), **_short(R.check(T, dst[i1], src[i2], f"tiled={tiled}"))}
        out[tiled] = T.tobytes()
    assert out[0] == out[2]
    _report("rigid_fit_icp_coplanar.json", report)


# ---- memory ---------------------------------------------------------------------------------------------------------------------
def test_nothing_stays_allocated(hip_lib):
    def live():
        out = (C.c_ulonglong * 2)()
        assert capi.load().cilhip_debug_live_allocations(out) == capi.OK
        return out[0], out[1]

    _, d, s = R.cases(0)[8]
    before = live()
    te = _est(d, s)
    te.estimateModel()
    te.countInliers(np.eye(4, dtype=F32)[None], THR)
    te.setMaxNumberOfIterations(3).setSeed(1).estimate()
    with pytest.raises(capi.CilhipError):
        _est(d, s).setSamples(np.array([[0, 1, 500]], np.uint32)).setMaxNumberOfIterations(1).estimate()
    assert live() == before
