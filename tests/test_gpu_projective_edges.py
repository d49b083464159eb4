"""GPU: projective association (csrc/projective.hip, run_projective_loop) on crafted scenes of a few thousand
points, where tests/test_gpu_projective.py runs two sensor frames: depth ties that only the original index can decide, projections
exactly on the edges rule P3 decides, the strict radius hit exactly, sizes around a block, one-pixel images -- indices exact and values
bit for bit against the numpy restatement (tests/_projective_refs.py; the scenes' own properties are pinned without a GPU in
tests/test_projective_refs_cpu.py) -- and every consumer of the stored set: the host estimates byte for byte against a grid context that
holds the same matches, the loop step by step for each metric, the weight evaluators, the post-filter, the convergence exit and an
iteration that finds nothing, against the oracle's update over the restated set.  TOL_T is the only tolerance."""
import collections
import ctypes as C

import numpy as np
import pytest

import _projective_refs as R
from test_gpu_estimate_entries import _affine, _combined, _p2p
from test_projective_refs_cpu import tie_group_span, tie_groups

pytestmark = pytest.mark.gpu

F = np.float32
TOL_T = 1e-5      # the project's bound on a transform (Frobenius)
I4 = np.eye(4, dtype=F)
W8, H6 = 8, 6
R2 = float(F(0.05) ** 2)      # the organized scene's radius
T_START = R.small_E(angles=(0.004, -0.003, 0.005), t=(0.004, -0.003, 0.002))      # the loops' start: small angles
# ... and a start far enough for a second and a third Gauss-Newton step to move the result (with its radius: fewer points project onto a match)
T_FAR, R2_FAR = R.small_E(angles=(0.12, -0.09, 0.15), t=(0.04, -0.03, 0.03)), float(F(0.1) ** 2)


def context(dst, nrm, src, K, w, h, E=None):
    from cilantro_amd.icp import Context

    ctx = Context(0)
    ctx.set_target(dst, nrm)
    ctx.set_source(src)
    if K is not None:
        ctx.set_projection(K, w, h, E)
    return ctx


def placed(a, memory):
    """the array itself, or a device-resident tensor of it"""
    if memory == "host":
        return a
    import torch

    return torch.from_numpy(np.array(a, F)).cuda()


def check(ctx, dst, src, T, max_sq, K, w, h, E=None):
    """one search against the restatement: the count, every index, the values' bits on the hits, the listed correspondences
    -> (the restated search, the engine's answer as bytes)"""
    want = R.projective_search(dst, src, T, max_sq, K, w, h, E)
    hit = np.flatnonzero(want[0] != R.EMPTY)
    assert ctx.find_correspondences(T, float(F(max_sq))) == hit.size
    idx, d2 = ctx.get_nn()
    assert np.array_equal(idx, want[0]), np.flatnonzero(idx != want[0])[:8]
    assert np.array_equal(d2[hit].view(np.uint32), want[1][hit].view(np.uint32))
    i1, i2, v = ctx.get_correspondences()      # ascending source index (S3)
    assert np.array_equal(i2, hit) and np.array_equal(i1, want[0][hit].astype(np.int64)) and np.array_equal(v.view(np.uint32), want[1][hit].view(np.uint32))
    return want, idx.tobytes() + d2.tobytes()


@pytest.fixture(scope="module")
def tie():
    """the tie scene, and a source of 300 of its points and the same points a dyadic step away"""
    pts, grp = R.tie_scene()
    sel = np.random.default_rng(11).choice(pts.shape[0], 300, replace=False)
    src = np.concatenate([pts[sel], pts[sel] + np.array([1 / 256, -1 / 256, 1 / 256], F)]).astype(F)
    for a in (pts, grp, src):
        a.setflags(write=False)
    return pts, grp, src


@pytest.fixture(scope="module")
def org():
    out = R.organized_scene()
    for a in out[:4]:
        a.setflags(write=False)
    return out


# ---- the index map and the search ----------------------------------------------------------------------------------------------------
E_HALF_TURN = np.array([[-1, 0, 0, 0.5], [0, -1, 0, -0.25], [0, 0, 1, 0.125], [0, 0, 0, 1]], F)      # a pose every product and sum of which is exact


@pytest.mark.parametrize("pose", ["identity", "small_E", "half_turn"])
@pytest.mark.parametrize("memory", ["host", "device"])
def test_depth_ties_go_to_the_lowest_original_index(tie, pose, memory):
    """rule P4 / S1: 64 points of bit-equal c_z per pixel, in an index order unrelated to the grid's.  Under the identity and under the
    half-turn pose (exact arithmetic: the ties survive the camera transform) every pixel is such a tie; under small_E rounding breaks most."""
    pts, grp, src = tie
    E = {"identity": None, "small_E": R.small_E(), "half_turn": E_HALF_TURN}[pose]
    dst, T = (pts, I4) if E is None else (R.transform(E[:3, :3], E[:3, 3], pts), E)
    if pose == "half_turn":
        assert np.array_equal(R.transform(*R.to_cam(E), dst), pts)      # the camera sees the scene's own coordinates, bit for bit
    if pose != "small_E":
        index = R.points_to_index_map(dst, R.TIE_K, W8, H6, E)
        assert all(index[p] == np.flatnonzero(grp == p).min() for p in range(W8 * H6))
    ctx = context(placed(dst, memory), None, placed(src, memory), R.TIE_K, W8, H6, E)
    # a tie group lies across several cells of the target's grid: within one cell the sorted order is the index order
    cell, span = float(ctx.grid_info().cell), tie_group_span(pts, tie_groups(pts))
    print(f"tie scene ({pose}, {memory}): grid cell {cell:.4f}, smallest extent of a tie group {span:.4f}")
    assert cell < span
    want, first = check(ctx, dst, src, T, 3e38, R.TIE_K, W8, H6, E)
    assert (want[0] != R.EMPTY).sum() >= 590      # (a nudged point may leave the image)
    _, again = check(ctx, dst, src, T, 3e38, R.TIE_K, W8, H6, E)
    assert first == again      # two runs: the same bytes
    near, _ = check(ctx, dst, src, T, 0.02, R.TIE_K, W8, H6, E)      # a radius that keeps a part: a point is matched to its pixel's winner, not to itself
    assert 50 < (near[0] != R.EMPTY).sum() < 550
    ctx.close()


def test_projections_on_the_edges_of_rule_p3_as_a_source():
    """u and v exactly -0.5, the float above it, 0.5, 1.5, 2.5, the float below w - 0.5, w - 0.5; |u| from 2^31 to inf; c_z of +-0, a
    denormal, NaN, inf; NaN coordinates: every pixel of the target holds points, so a source point is matched iff rule P3 accepts it"""
    dst = R.tie_scene(K=R.EDGE_K)[0]
    src, pixel = R.boundary_points(W8, H6)
    index = R.points_to_index_map(dst, R.EDGE_K, W8, H6)
    assert (index != R.EMPTY).all()
    ctx = context(dst, None, src, R.EDGE_K, W8, H6)
    want, _ = check(ctx, dst, src, I4, 3e38, R.EDGE_K, W8, H6)
    idx = ctx.get_nn()[0]
    assert np.array_equal(idx != R.EMPTY, pixel >= 0) and np.array_equal(idx[pixel >= 0], index[pixel[pixel >= 0]])
    assert (pixel >= 0).sum() == 3 * 14
    ctx.close()


def test_projections_on_the_edges_of_rule_p3_inside_a_target():
    """the same points as map points: the map the search reads is the restated map, and the boundary points that win a pixel are found"""
    bnd = R.boundary_points(W8, H6)[0]
    bnd = bnd[~((np.abs(bnd) > 1e30) & np.isfinite(bnd)).any(axis=1)]      # (finite coordinates near FLT_MAX: the grid refuses such a target; 2^38, NaN and inf stay)
    assert bnd.shape[0] == 76 and np.isnan(bnd).any() and np.isinf(bnd).any()
    tie_pts = R.tie_scene(K=R.EDGE_K)[0]
    dst = np.concatenate([bnd, tie_pts[::8]])      # the boundary points first: they win the depth ties of the pixels they land on
    src = np.concatenate([tie_pts[:300], bnd])
    index = R.points_to_index_map(dst, R.EDGE_K, W8, H6)
    assert ((index != R.EMPTY) & (index < bnd.shape[0])).sum() >= 8      # boundary points hold pixels of the map
    ctx = context(dst, None, src, R.EDGE_K, W8, H6)
    want, _ = check(ctx, dst, src, I4, 3e38, R.EDGE_K, W8, H6)
    assert ((want[0] != R.EMPTY) & (want[0] < bnd.shape[0])).sum() >= 50
    check(ctx, dst, src, I4, 1e-3, R.EDGE_K, W8, H6)
    ctx.close()


def test_the_radius_is_strict():
    """q - p = (0.25, 0, 0) on one pixel: value = 0.0625 exactly; kept iff 0.0625 < max_sq_dist"""
    p = np.array([[-0.375, -0.25, 2.0], [0.5, 0.25, 1.0], [-1.0, 0.5, 2.0]], F)      # u = 2.75, v = 2 at z = 2; two points elsewhere
    q = (p[:1] + np.array([0.25, 0, 0], F)).astype(F)                                 # u = 3.25: the same pixel
    assert R.project(p[:1], R.TIE_K, W8, H6)[1][0] == R.project(q, R.TIE_K, W8, H6)[1][0] == 2 * W8 + 3
    ctx = context(p, None, q, R.TIE_K, W8, H6)
    edge = F(0.0625)
    for max_sq, found in ((edge, 0), (np.nextafter(edge, F(1)), 1), (np.nextafter(edge, F(0)), 0), (F(1.0), 1)):
        want, _ = check(ctx, p, q, I4, float(max_sq), R.TIE_K, W8, H6)
        assert int((want[0] != R.EMPTY).sum()) == found, max_sq
        assert ctx.find_correspondences(I4, float(max_sq)) == found
        if found:
            assert ctx.get_nn()[1].view(np.uint32)[0] == edge.view(np.uint32)
    ctx.close()


@pytest.mark.parametrize("memory", ["host", "device"])
def test_sizes_around_a_block(org, memory):
    P, N, S, K, w, h = org
    dev = lambda a: placed(a, memory)      # noqa: E731
    T = T_START
    ctx = context(dev(P), dev(N), dev(S[:1]), K, w, h)
    for ns in (1, 255, 256, 257):
        ctx.set_source(dev(S[:ns]))
        for Tk in (I4, T):
            want, _ = check(ctx, P, S[:ns], Tk, R2, K, w, h)
            assert (want[0] != R.EMPTY).sum() >= ns - 3
    for nt in (1, 255, 256, 257):
        ctx.set_target(dev(P[:nt]), dev(N[:nt]))
        want, _ = check(ctx, P[:nt], S[:257], I4, R2, K, w, h)
        assert (want[0] != R.EMPTY).sum() == (nt + 2) // 3      # the source points whose own target point is there
    ctx.close()


@pytest.mark.parametrize("w,h", [(1, 1), (1, 6), (8, 1)])
def test_one_pixel_wide_images(tie, w, h):
    """the tie scene seen by a camera whose principal point is pixel (0, 0): a part of it lands inside a 1 x 1, a 1 x 6 and an 8 x 1 image"""
    pts, _, src = tie
    ctx = context(pts, None, src, R.EDGE_K, w, h)
    want, _ = check(ctx, pts, src, I4, 3e38, R.EDGE_K, w, h)
    n = int((want[0] != R.EMPTY).sum())
    print(f"{w} x {h}: {n} of {src.shape[0]} source points matched")
    assert 10 < n < src.shape[0]
    ctx.close()


def test_a_source_without_a_finite_point(tie):
    pts = tie[0]
    src = np.array([[np.nan, 0, 1], [0, np.inf, 1], [0, 0, np.nan], [-np.inf, np.nan, np.inf], [np.inf, np.inf, np.inf]], F)
    ctx = context(pts, None, src, R.TIE_K, W8, H6)
    want, _ = check(ctx, pts, src, I4, 3e38, R.TIE_K, W8, H6)
    assert (want[0] == R.EMPTY).all() and ctx.find_correspondences(R.small_E(), 3e38) == 0
    ctx.close()


# ---- the consumers of the stored set -------------------------------------------------------------------------------------------------
RBF = (("point_weight_evaluator", 2), ("plane_weight_evaluator", 2), ("point_weight_sigma", 0.05), ("plane_weight_sigma", 0.08))


def test_estimates_over_a_projective_set_are_those_over_the_same_grid_set(org):
    """everything that reads the last search works unchanged.  On the organized scene the projective search and the grid
    search hold the same matches (asserted; proved on the CPU), so the host estimates -- f64 in a fixed order -- must give the same BYTES"""
    P, N, S, K, w, h = org
    proj, grid = context(P, N, S, K, w, h), context(P, N, S, None, w, h)
    assert proj.find_correspondences(I4, R2) == grid.find_correspondences(I4, R2) == S.shape[0]
    a, b = proj.get_nn(), grid.get_nn()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(proj.get_correspondences(), grid.get_correspondences()))
    compared, first_step = 0, []
    for evaluators in ((), RBF):
        for ctx in (proj, grid):
            for k, v in evaluators:
                ctx.set_option(k, v)
        results = []
        for ctx in (proj, grid):
            out = {"p2p": _p2p(ctx)}
            for wt in ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7)):
                for it in (0, 1, 5):
                    out[f"combined {wt} it={it}"] = _combined(ctx, wt, it)
                for centered in (True, False):
                    out[f"affine {wt} centered={centered}"] = _affine(ctx, wt, centered)
            results.append(out)
        differ = [k for k in results[0] if results[0][k].tobytes() != results[1][k].tobytes()]
        assert not differ, (bool(evaluators), differ)
        compared += len(results[0])
        # (the estimates did estimate: the source is a step away from the target)
        assert not np.array_equal(np.frombuffer(results[0]["combined (0.3, 0.7) it=1"].tobytes()[:64], F), I4.reshape(16))
        assert not np.array_equal(np.frombuffer(results[0]["p2p"].tobytes()[:64], F), I4.reshape(16))
        first_step.append(results[0]["combined (0.3, 0.7) it=1"].tobytes())
    assert compared == 2 * (1 + 9 + 6)
    assert first_step[0] != first_step[1]      # the evaluators changed the estimate
    proj.close()
    grid.close()


Variant = collections.namedtuple("Variant", "metric w_p2p w_p2pl steps sigmas fraction start radius", defaults=(None, 1.0, T_START, R2))
VARIANTS = {"point_to_point": Variant(0, 0.0, 1.0, 1), "plane_only": Variant(1, 0.0, 1.0, 1),
            "combined_3_steps": Variant(1, 0.2, 1.0, 3, start=T_FAR, radius=R2_FAR),
            "rbf_evaluators": Variant(1, 0.3, 0.7, 1, sigmas=(0.01, 0.02)), "inlier_fraction": Variant(1, 0.0, 1.0, 1, fraction=0.5)}


def loop_params(v, max_iter, conv_tol, max_sq_dist=None):
    from cilantro_amd import capi

    p = capi.IcpParams()
    capi.load().cilhip_icp_default_params(C.byref(p))
    p.metric, p.w_p2p, p.w_p2pl, p.max_iter, p.conv_tol, p.max_opt_iter, p.opt_conv_tol = v.metric, v.w_p2p, v.w_p2pl, max_iter, conv_tol, v.steps, 1e-6
    p.max_sq_dist = v.radius if max_sq_dist is None else max_sq_dist
    return p


def variant_context(org, v):
    P, N, S, K, w, h = org
    ctx = context(P, N, S, K, w, h)
    if v.sigmas:
        for key, value in (("point_weight_evaluator", 2), ("plane_weight_evaluator", 2), ("point_weight_sigma", v.sigmas[0]), ("plane_weight_sigma", v.sigmas[1])):
            ctx.set_option(key, value)
    if v.fraction < 1.0:
        ctx.set_option("inlier_fraction", v.fraction)
    return ctx


def oracle_params(orc, v, steps=None):
    kw = dict(point_weight=orc.W_RBF, plane_weight=orc.W_RBF, point_sigma=v.sigmas[0], plane_sigma=v.sigmas[1]) if v.sigmas else {}
    return orc.make_params(metric=v.metric, w_p2p=v.w_p2p, w_p2pl=v.w_p2pl, max_iter=1, conv_tol=0.0, max_opt_iter=v.steps if steps is None else steps, opt_conv_tol=1e-6,
                           max_sq_dist=v.radius, **kw)


def restated_set(orc, org, T, max_sq_dist, fraction=1.0):
    """the correspondences one iteration works on: the restated search under T, through the oracle's fraction filter where one is set
    -> (target indices, source indices, values)"""
    P, N, S, K, w, h = org
    nn, val = R.projective_search(P, S, T, max_sq_dist, K, w, h)
    src = np.flatnonzero(nn != R.EMPTY)
    di, si, dv = nn[src].astype(np.int64), src, val[src]
    return orc.filter_fraction(di, si, dv, fraction) if fraction < 1.0 else (di, si, dv)


def frobenius(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - np.asarray(b, np.float64)))


@pytest.mark.parametrize("max_iter", [1, 2, 3])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_loop_step_by_step(org, orc, name, max_iter):
    """conv_tol = 0: after max_iter iterations the stored matches are the restated search under the transform of the last search (through
    the oracle's filter where one is set), and the oracle's update over that set from that transform is the engine's result.

    What each part can tell apart: the stored set, its order, its values, the origin and last_ncorr are exact in every row.  The transform
    is compared over ONE update, from the engine's own matches_transform(); at max_iter = 1 that update is large and the variants' updates
    lie far apart (RBF against unity 1.9e-3, point-to-point against plane 5.1e-3 on this scene), at max_iter 2 and 3 the small-angle rows are
    nearly converged and every variant's last update agrees to about 1e-7: there the exact checks carry the row, not the transform.  The
    row with three Gauss-Newton steps starts far away so that the steps matter in all three rows, and asserts that they do: the oracle's
    results after one, two and three steps over the same set lie well over TOL_T apart before the engine is compared with the third."""
    P, N, S, K, w, h = org
    v = VARIANTS[name]
    ctx = variant_context(org, v)
    res = ctx.icp_run(loop_params(v, max_iter, 0.0), v.start)
    assert res.iterations == max_iter
    Tm = ctx.matches_transform()
    if max_iter == 1:
        assert np.array_equal(Tm, v.start)
    di, si, dv = restated_set(orc, org, Tm, v.radius, v.fraction)
    i1, i2, val = ctx.get_correspondences()
    assert np.array_equal(i1, di) and np.array_equal(i2, si) and np.array_equal(val.view(np.uint32), dv.view(np.uint32))
    assert ctx.last_matches_origin() == (2 if v.fraction < 1.0 else 1)      # a filtered set is searched again on demand, projectively
    assert res.last_ncorr == len(di) > 300
    if v.fraction < 1.0:
        assert len(di) < 0.6 * restated_set(orc, org, Tm, v.radius)[0].size      # (the filter did remove matches)
    T_orc, _ = orc.icp_update(P, N, S, Tm, di, si, oracle_params(orc, v), values=dv)
    T_gpu = np.array(res.T, F).reshape(4, 4).T
    if v.steps > 1:
        fewer = [orc.icp_update(P, N, S, Tm, di, si, oracle_params(orc, v, steps), values=dv)[0] for steps in range(1, v.steps)]
        apart = [frobenius(T, T_orc) for T in fewer]
        print(f"{name} max_iter={max_iter}: the oracle after 1 .. {v.steps - 1} steps is {', '.join('%.2e' % a for a in apart)} from its result after {v.steps}")
        assert apart[0] > (100 if max_iter == 1 else 5) * TOL_T      # one step alone would be told from three ...
        if max_iter == 1:
            assert apart[-1] > 10 * TOL_T      # ... and so would two
    err = frobenius(T_gpu, T_orc)
    print(f"{name} max_iter={max_iter}: n = {len(di)}, |T_gpu - T_oracle|_F = {err:.3e}")
    assert err <= TOL_T
    if max_iter == 1:
        assert frobenius(T_gpu, Tm) > 100 * TOL_T      # (the first step is a step)
    ctx.close()


@pytest.mark.parametrize("name,stops_after", [("plane_only", 2), ("point_to_point", 3)])
def test_convergence_exit(org, orc, name, stops_after):
    """conv_tol = 1e-3 and up to 6 iterations against the yardstick loop (restated search + the oracle's update): the same number of
    iterations, the same transform.  The yardstick's update norms are far from the tolerance on both sides (asserted), so the count cannot
    hinge on the last bits"""
    P, N, S, K, w, h = org
    v = VARIANTS[name]
    tol = 1e-3
    T, iters, deltas = v.start, 0, []
    while iters < 6:
        di, si, dv = restated_set(orc, org, T, v.radius, v.fraction)
        T, delta = orc.icp_update(P, N, S, T, di, si, oracle_params(orc, v), values=dv)
        iters += 1
        deltas.append(delta)
        if delta < tol:
            break
    assert iters == stops_after and all(d > 2 * tol for d in deltas[:-1]) and deltas[-1] < tol / 2, deltas
    ctx = variant_context(org, v)
    res = ctx.icp_run(loop_params(v, 6, tol), v.start)
    err = frobenius(np.array(res.T, F).reshape(4, 4).T, T)
    print(f"{name}: iterations gpu={res.iterations} yardstick={iters}, update norms {deltas}, |T_gpu - T_yardstick|_F = {err:.3e}")
    assert res.iterations == iters and res.last_ncorr == len(di)
    assert err <= TOL_T
    ctx.close()


@pytest.mark.parametrize("name", ["plane_only", "point_to_point", "inlier_fraction"])
@pytest.mark.parametrize("conv_tol,iterations", [(0.0, 3), (1e-6, 1)])
def test_iterations_that_find_nothing(org, orc, name, conv_tol, iterations):
    """max_sq_dist = 1e-14: no source point has a match.  The oracle's update over the empty set leaves the transform as it is with an update
    norm of 0 (pinned on the CPU), so the yardstick loop runs every iteration under conv_tol = 0 and one under any positive tolerance"""
    P, N, S, K, w, h = org
    v = VARIANTS[name]
    none = np.zeros(0, np.int64)
    assert restated_set(orc, org, v.start, 1e-14)[0].size == 0
    T_orc, delta = orc.icp_update(P, N, S, v.start, none, none, oracle_params(orc, v))
    assert delta == 0.0
    ctx = variant_context(org, v)
    res = ctx.icp_run(loop_params(v, 3, conv_tol, max_sq_dist=1e-14), v.start)
    err = frobenius(np.array(res.T, F).reshape(4, 4).T, T_orc)
    print(f"{name}, nothing found, conv_tol={conv_tol}: iterations {res.iterations}, update norm {res.last_delta_norm}, |T_gpu - T_oracle|_F = {err:.3e}")
    assert res.iterations == iterations and res.last_ncorr == 0 and res.last_delta_norm == 0.0
    assert err <= TOL_T
    assert (ctx.get_nn()[0] == R.EMPTY).all() and ctx.get_correspondences()[0].size == 0
    ctx.close()
