"""GPU: projective association inside a context (cilhip_set_projection) against the numpy restatement of
tests/_projective_refs.py -- indices and values bit for bit -- and the projective ICP loop, step by step, against the oracle's update
over the restated correspondence set."""
import ctypes as C

import numpy as np
import pytest

import _projective_refs as R
from test_projective_refs_cpu import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32
TOL_T = 1e-5      # the project's bound on a transform (Frobenius)
E_SMALL = R.small_E()
T_SMALL = R.small_E(angles=(0.01, -0.008, 0.012), t=(0.01, -0.005, 0.008))


@pytest.fixture(scope="module")
def frames():
    d = np.load(GOLDEN)
    out = (d["p1"], d["n1"], d["p2"])
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def identity_search(frames):
    """the restated search of p2 against p1 under the identity at the three radii of DESIGN 14.4 (computed once)"""
    return {r: R.projective_search(frames[0], frames[2], np.eye(4, dtype=F), F(r) ** 2, K=R.FUSION_K) for r in (0.01, 0.02, 0.1)}


def context(dst, nrm, src, K=R.FUSION_K, E=None, w=640, h=480):
    from cilantro_amd.icp import Context

    ctx = Context(0)
    ctx.set_target(dst, nrm)
    ctx.set_source(src)
    if K is not None:
        ctx.set_projection(K, w, h, E)
    return ctx


def params(max_iter, conv_tol, max_sq_dist):
    from cilantro_amd import capi

    p = capi.IcpParams()
    capi.load().cilhip_icp_default_params(C.byref(p))
    p.metric, p.w_p2p, p.w_p2pl, p.max_iter, p.conv_tol, p.max_opt_iter, p.max_sq_dist = capi.METRIC_COMBINED, 0.0, 1.0, max_iter, conv_tol, 1, max_sq_dist
    return p


def same_search(ctx, want):
    idx, d2 = ctx.get_nn()
    assert np.array_equal(idx, want[0])
    hit = want[0] != R.EMPTY
    assert np.array_equal(d2[hit].view(np.uint32), want[1][hit].view(np.uint32))


def test_restated_counts(identity_search):
    assert [int((identity_search[r][0] != R.EMPTY).sum()) for r in (0.01, 0.02, 0.1)] == [61494, 75079, 108515]


@pytest.mark.parametrize("r", [0.01, 0.1])
def test_search_identity_and_rigid(frames, identity_search, r):
    p1, n1, p2 = frames
    ctx = context(p1, n1, p2)
    r2 = float(F(r) ** 2)
    assert ctx.find_correspondences(np.eye(4, dtype=F), r2) == int((identity_search[r][0] != R.EMPTY).sum())
    same_search(ctx, identity_search[r])
    want = R.projective_search(p1, p2, T_SMALL, r2, K=R.FUSION_K)
    assert ctx.find_correspondences(T_SMALL, r2) == int((want[0] != R.EMPTY).sum()) > 1000
    same_search(ctx, want)
    i1, i2, v = ctx.get_correspondences()      # ascending source index (S3)
    hit = np.flatnonzero(want[0] != R.EMPTY)
    assert np.array_equal(i2, hit) and np.array_equal(i1, want[0][hit].astype(np.int64)) and np.array_equal(v, want[1][hit])
    ctx.close()


def test_search_world_frame_model(frames):
    """the model in the world frame, the camera posed at E: the source frame enters with T = E"""
    p1, n1, p2 = frames
    world = R.transform(E_SMALL[:3, :3], E_SMALL[:3, 3], p1)
    ctx = context(world, None, p2, E=E_SMALL)
    want = R.projective_search(world, p2, E_SMALL, F(0.02) ** 2, K=R.FUSION_K, E=E_SMALL)
    assert ctx.find_correspondences(E_SMALL, float(F(0.02) ** 2)) == int((want[0] != R.EMPTY).sum()) > 50000
    same_search(ctx, want)
    ctx.close()


def test_search_inlier_fraction(frames, identity_search, orc):
    p1, n1, p2 = frames
    ctx = context(p1, n1, p2)
    ctx.set_option("inlier_fraction", 0.5)
    n = ctx.find_correspondences(np.eye(4, dtype=F), float(F(0.02) ** 2))
    nn, val = identity_search[0.02]
    src = np.flatnonzero(nn != R.EMPTY)
    di, si, dv = orc.filter_fraction(nn[src].astype(np.int64), src, val[src], 0.5)
    assert n == len(di) and 0 < n < src.size
    i1, i2, v = ctx.get_correspondences()
    assert np.array_equal(i1, di) and np.array_equal(i2, si) and np.array_equal(v, dv)      # (the kept set, in the filter's order: by value)
    ctx.close()


def test_search_edge_cases(frames):
    p1, n1, p2 = frames
    ctx = context(p1, n1, np.zeros((0, 3), F))      # ns = 0
    assert ctx.find_correspondences(np.eye(4, dtype=F), 0.01) == 0
    ctx.close()
    behind = (p1 * np.array([1, 1, -1], F)).astype(F)      # a target entirely behind the camera
    ctx = context(behind, None, p2[:5000])
    assert ctx.find_correspondences(np.eye(4, dtype=F), 100.0) == 0
    assert (ctx.get_nn()[0] == R.EMPTY).all()
    # a small image and the default camera of the engine's mirror: most of the cloud projects outside
    ctx.set_projection(R.DEFAULT_K, 67, 45)
    ctx.set_target(p1[:20000], None)
    want = R.projective_search(p1[:20000], p2[:5000], np.eye(4, dtype=F), 0.01, K=R.DEFAULT_K, w=67, h=45)
    assert ctx.find_correspondences(np.eye(4, dtype=F), 0.01) == int((want[0] != R.EMPTY).sum())
    same_search(ctx, want)
    ctx.close()


def T_start():
    return R.small_E(angles=(0.004, -0.003, 0.005), t=(0.004, -0.003, 0.002))


@pytest.mark.parametrize("max_iter", [1, 2, 3, 4])
def test_loop_step_by_step(frames, orc, max_iter):
    """conv_tol = 0: after max_iter iterations the stored matches are the restatement's search under the transform of the last search,
    and the oracle's update over that set from that transform is the engine's result"""
    p1, n1, p2 = frames
    r2 = float(F(0.05) ** 2)
    ctx = context(p1, n1, p2)
    res = ctx.icp_run(params(max_iter, 0.0, r2), T_start())
    assert res.iterations == max_iter
    Tm = ctx.matches_transform()
    want = R.projective_search(p1, p2, Tm, r2, K=R.FUSION_K)
    same_search(ctx, want)
    assert ctx.last_matches_origin() == 1
    src = np.flatnonzero(want[0] != R.EMPTY)
    assert res.last_ncorr == src.size > 50000
    T_orc, _ = orc.icp_update(p1, n1, p2, Tm, want[0][src].astype(np.int64), src, orc.make_params(metric=1, max_iter=1, conv_tol=0.0, max_sq_dist=r2))
    T_gpu = np.array(res.T, F).reshape(4, 4).T
    err = float(np.linalg.norm(T_gpu.astype(np.float64) - T_orc.astype(np.float64)))
    print(f"max_iter={max_iter}: |T_gpu - T_oracle|_F = {err:.3e}")
    assert err <= TOL_T
    ctx.close()


def test_fusion_settings_end_to_end(frames, orc):
    """examples/fusion.cpp:127-158: max_distance 0.1^2, 6 iterations, tolerance 5e-4, through the mirror class, against the yardstick loop
    (restated search + the oracle's update)"""
    from cilantro_amd.icp import SimpleCombinedMetricRigidProjectiveICP3f

    p1, n1, p2 = frames
    r2 = float(F(0.1) ** 2)
    icp = SimpleCombinedMetricRigidProjectiveICP3f(p1, n1, p2)
    eng = icp.correspondenceSearchEngine()
    assert eng.getProjectionImageWidth() == 640 and eng.getProjectionImageHeight() == 480 and eng.getProjectionIntrinsicMatrix()[0, 0] == 528
    eng.setProjectionIntrinsicMatrix(R.FUSION_K).setMaxDistance(r2)
    icp.setInitialTransform(T_start()).setMaxNumberOfIterations(6).setConvergenceTolerance(5e-4)
    T_gpu = icp.estimate().getTransform()
    T, iters = T_start(), 0
    prm = orc.make_params(metric=1, max_iter=1, conv_tol=0.0, max_sq_dist=r2)
    while iters < 6:
        nn, _ = R.projective_search(p1, p2, T, r2, K=R.FUSION_K)
        src = np.flatnonzero(nn != R.EMPTY)
        T, delta = orc.icp_update(p1, n1, p2, T, nn[src].astype(np.int64), src, prm)
        iters += 1
        if delta < 5e-4:
            break
    err = float(np.linalg.norm(T_gpu.astype(np.float64) - T.astype(np.float64)))
    print(f"fusion settings: iterations gpu={icp.getNumberOfPerformedIterations()} yardstick={iters} |T_gpu - T_yardstick|_F = {err:.3e}")
    assert icp.getNumberOfPerformedIterations() == iters
    assert err <= TOL_T


def test_lifecycle_and_repeat_runs(frames):
    p1, n1, p2 = frames
    sub = p2[:30000]
    r2 = float(F(0.02) ** 2)
    I = np.eye(4, dtype=F)
    ctx = context(p1, n1, sub)
    ctx.find_correspondences(I, r2)
    a = ctx.get_nn()
    ctx.find_correspondences(I, r2)
    b = ctx.get_nn()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()      # two runs: the same bits
    # a new target rebuilds the map
    ctx.set_target(p1[::2].copy(), n1[::2].copy())
    ctx.find_correspondences(I, r2)
    same_search(ctx, R.projective_search(p1[::2], sub, I, r2, K=R.FUSION_K))
    # a new projection rebuilds it too
    ctx.set_projection(R.FUSION_K, 640, 480, E_SMALL)
    ctx.find_correspondences(I, r2)
    same_search(ctx, R.projective_search(p1[::2], sub, I, r2, K=R.FUSION_K, E=E_SMALL))
    # a borrowed target has a map of its own
    other = context(p1, n1, sub, K=None)
    ctx.share_target(other)
    ctx.find_correspondences(I, r2)
    same_search(ctx, R.projective_search(p1, sub, I, r2, K=R.FUSION_K, E=E_SMALL))
    # no projection: a fresh context's grid results
    ctx.set_projection(None)
    n_grid = ctx.find_correspondences(I, r2)
    fresh = context(p1, n1, sub, K=None)
    assert fresh.find_correspondences(I, r2) == n_grid
    g, f = ctx.get_nn(), fresh.get_nn()
    assert np.array_equal(g[0], f[0]) and np.array_equal(g[1][g[0] != R.EMPTY], f[1][f[0] != R.EMPTY])
    res_a, res_b = ctx.icp_run(params(3, 0.0, r2)), fresh.icp_run(params(3, 0.0, r2))
    assert bytes(res_a.T) == bytes(res_b.T)
    for c in (ctx, other, fresh):
        c.close()


def test_refused_combinations(frames):
    from cilantro_amd import capi

    p1, n1, p2 = frames
    ctx = context(p1[:5000], n1[:5000], p2[:3000])
    I = np.eye(4, dtype=F)

    def refused(call):
        with pytest.raises(capi.CilhipError) as e:
            call()
        assert e.value.code == capi.ERR_UNSUPPORTED and "projective" in str(e.value), str(e.value)

    both = (lambda: ctx.find_correspondences(I, 0.01), lambda: ctx.icp_run(params(2, 0.0, 0.01)))
    for key, bad, good in (("search_direction", 1, 0), ("search_direction", 2, 0), ("one_to_one", 1, 0), ("feature_normal_weight", 0.5, 0.0)):
        ctx.set_option(key, bad)
        for call in both:
            refused(call)
        ctx.set_option(key, good)
    ctx.set_option("search_direction", 2)
    ctx.set_option("require_reciprocality", 1)
    refused(both[0])
    ctx.set_option("require_reciprocality", 0)
    ctx.set_option("search_direction", 0)
    ctx.set_pair_weight_callback(lambda i1, i2, v: (np.ones_like(v), np.ones_like(v)))
    for call in both:
        refused(call)
    ctx.set_pair_weight_callback(None)
    ctx.set_option("transform_mode", 1)      # the affine loop
    refused(both[1])
    ctx.set_option("transform_mode", 0)
    refused(lambda: ctx.icp_begin(params(2, 0.0, 0.01)))      # the sharded building blocks (cilhip_multi_* run through them)
    ctx.set_shard_info(16)      # a target shard
    for call in both:
        refused(call)
    ctx.set_shard_info(0)
    other = context(p1[:5000], n1[:5000], p2[:3000], K=None)
    res = capi.IcpResult()
    p = params(2, 0.0, 0.01)
    for a, b in ((ctx, other), (other, ctx)):
        rc = ctx._L.cilhip_icp_run_two_sets(a._h, C.c_float(0.01), b._h, C.c_float(0.01), C.byref(p), None, C.byref(res))
        assert rc == capi.ERR_UNSUPPORTED and b"projective" in ctx._L.cilhip_last_error(a._h)
    # ... and with everything back in place the projective search runs, cilhip_compute_residuals untouched by the projection
    assert ctx.find_correspondences(I, 0.01) >= 0
    assert ctx.icp_run(params(2, 0.0, 0.01)).iterations == 2
    r_proj = ctx.compute_residuals(1, 0.0, 1.0, I)
    assert np.array_equal(r_proj, other.compute_residuals(1, 0.0, 1.0, I), equal_nan=True)
    ctx.close()
    other.close()
