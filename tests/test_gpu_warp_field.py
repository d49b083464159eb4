"""GPU: the warp-field entries of c_api.h against tests/_warp_refs.py, through the C ABI.

Yardsticks: the f64 restatement is "the exact answer", the f32 restatement "the reference as it runs"; a tolerance is the f32
restatement's own error against the f64 one on the same inputs, times 4 (slack for a different but equally valid summation order), per
component class (a, b, c, tx, ty, tz: the maximum over the control nodes).  The device's tforms_vec is read back through the transforms
(angles of Rz Ry Rx, translation); the f32 restatement goes through the same read-back (f32 transforms) before it is measured.

Shapes: a curved surface, 3 000 source / 4 000 target points, the target bent by ~4 mm; 204 control nodes (not a multiple of 64, more
than one block of nodes, ragged lists at the border), k_ctrl = 4, k_reg = 8; one case with 70 000 source points (more than one grid
trip of the per-point kernels: 256 blocks x 256 lanes).

Note on the Huber case: at the first Gauss-Newton step tforms_vec is 0, every regularisation difference is 0 and only the quadratic
branch can occur; the case therefore runs TWO Gauss-Newton steps (each with 1, then 2 CG iterations) so that the second linearisation
meets both branches; the restatement asserts that it does.

Figures of the first MI355X run are recorded in the docstrings of the tests that measure them."""
import ctypes as C

import numpy as np
import pytest

import _warp_refs as W
from cilantro_amd import capi

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
HOST = capi.MEM_HOST


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def last_error(L):
    return L.cilhip_last_error(None).decode()


class Field:
    def __init__(self, n_src, n_ctrl, ctrl_idx, ctrl_d2, ctrl_kernel, ctrl_sigma, reg_idx, reg_d2, reg_kernel, reg_sigma):
        self.L = capi.load()
        self.n_src, self.n_ctrl = n_src, n_ctrl
        ci, cd, ri, rd = np.ascontiguousarray(ctrl_idx, np.uint32), np.ascontiguousarray(ctrl_d2, F), np.ascontiguousarray(reg_idx, np.uint32), np.ascontiguousarray(reg_d2, F)
        self.h = C.c_void_p()
        rc = self.L.cilhip_warp_field_create(0, n_src, n_ctrl, ci.ctypes.data, cd.ctypes.data, ci.shape[1], ctrl_kernel, float(ctrl_sigma), ri.ctypes.data, rd.ctypes.data, ri.shape[1],
                                             reg_kernel, float(reg_sigma), HOST, C.byref(self.h))
        assert rc == capi.OK, last_error(self.L)

    @classmethod
    def of(cls, c):
        return cls(len(c["src"]), c["n_ctrl"], c["ctrl_idx"], c["ctrl_d2"], c["ctrl_kernel"], c["ctrl_sigma"], c["reg_idx"], c["reg_d2"], c["reg_kernel"], c["reg_sigma"])

    def close(self):
        self.L.cilhip_warp_field_destroy(self.h)

    def estimate(self, dst, nrm, src, nn, p, expect=capi.OK):
        dst, src, nn = np.ascontiguousarray(dst, F), np.ascontiguousarray(src, F), np.ascontiguousarray(nn, np.uint32)
        nrm = None if nrm is None else np.ascontiguousarray(nrm, F)
        out, st = np.full(16 * self.n_ctrl, 7, F), capi.WarpStats()
        rc = self.L.cilhip_warp_field_estimate3f(self.h, dst.ctypes.data, None if nrm is None else nrm.ctypes.data, len(dst), src.ctypes.data, nn.ctypes.data, HOST, C.byref(cparams(p)),
                                                 out.ctypes.data, C.byref(st))
        assert rc == expect, last_error(self.L)
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), st, out.tobytes()

    def resample(self, T):
        t = np.ascontiguousarray(np.asarray(T, F).transpose(0, 2, 1)).reshape(-1)
        out = np.zeros(16 * self.n_src, F)
        assert self.L.cilhip_warp_field_resample3f(self.h, t.ctypes.data, out.ctypes.data, HOST) == capi.OK, last_error(self.L)
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()


def cparams(p):
    return capi.WarpParams(float(p.w_p2p), float(p.w_p2pl), float(p.w_reg), float(p.huber_boundary), p.max_gn_iter, float(p.gn_conv_tol), p.max_cg_iter, float(p.cg_conv_tol))


def transform_points(T, xyz):
    L = capi.load()
    t, p = np.ascontiguousarray(np.asarray(T, F).transpose(0, 2, 1)).reshape(-1), np.ascontiguousarray(xyz, F)
    out = np.zeros_like(p)
    assert L.cilhip_transform_points_per_point3f(0, t.ctypes.data, p.ctypes.data, len(p), HOST, out.ctypes.data) == capi.OK, last_error(L)
    return out


def prm(**kw):
    """the example's parameters (examples/non_rigid_icp.cpp:75-82)"""
    base = dict(w_p2p=0.0, w_p2pl=1.0, w_reg=200.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=500, cg_conv_tol=1e-5)
    base.update(kw)
    return W.Params(**base)


def readback(T):
    """(a, b, c, tx, ty, tz) per node, f64, from transforms"""
    return np.concatenate([W.angles_of(T), np.asarray(T, D)[:, :3, 3]], 1)


def component_errors(T, exact_tf):
    return np.abs(readback(T) - np.asarray(exact_tf, D).reshape(-1, 6)).max(0)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    c = W.make_case()
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    assert 150 <= c["n_ctrl"] <= 300 and c["n_ctrl"] % 64 != 0
    assert (c["nn"] != W.NONE).sum() > 2000
    return c


@pytest.fixture(scope="module")
def field(case):
    f = Field.of(case)
    yield f
    f.close()


_REFS = {}


def refs(case, p, key):
    """the f32 and f64 restatements of one estimate, computed once per parameter set"""
    if key not in _REFS:
        out = {}
        for t in (F, D):
            rec = []
            tf, st = W.estimate(case["graph"], t, case["dst"], case["dst_n"], case["src"], case["nn"], p, record=rec)
            out[t] = dict(tf=tf, st=st, rec=rec)
        _REFS[key] = out
    return _REFS[key]


ASSEMBLY = {"plane": dict(), "point_and_plane": dict(w_p2p=0.1), "huber_two_steps": dict(w_p2p=0.1, huber_boundary=2e-5, max_gn_iter=2, gn_conv_tol=0.0)}


# ---- 1. assembly, isolated from convergence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("name", list(ASSEMBLY))
def test_assembly_after_one_and_two_cg_iterations(case, field, name, max_cg):
    """x1 = alpha M^-1 A^T b exercises A^T b, the diagonal and one operator application; x2 one more.
    First MI355X run, errors against the f64 restatement per component class (a, b, c, tx, ty, tz), f32 restatement / device:
      plane, 1 CG iteration            1.9e-8 3.7e-8 7.6e-9 3.0e-11 3.1e-11 1.1e-10  /  3.3e-11 3.7e-11 1.8e-11 1.7e-11 1.4e-11 5.4e-11
      plane, 2                         7.7e-9 2.4e-8 2.1e-9 9.4e-11 5.0e-11 1.9e-10  /  5.3e-11 4.4e-11 1.9e-11 2.4e-11 1.7e-11 7.8e-11
      point and plane, 1               9.5e-9 3.2e-8 1.4e-8 4.7e-11 4.9e-11 1.4e-10  /  6.7e-11 6.3e-11 2.3e-11 3.2e-11 2.5e-11 1.2e-10
      point and plane, 2               5.5e-9 2.6e-8 4.6e-9 8.1e-11 6.1e-11 2.7e-10  /  1.1e-10 9.3e-11 3.0e-11 3.8e-11 4.4e-11 1.6e-10
      Huber, two steps of 1            1.9e-8 6.4e-8 6.3e-10 7.4e-10 2.6e-10 4.2e-9  /  3.3e-9 3.4e-9 2.3e-10 7.5e-10 2.6e-10 4.2e-9
      Huber, two steps of 2            4.8e-9 1.0e-8 3.8e-10 7.0e-10 5.4e-10 5.8e-9  /  1.8e-9 1.5e-9 4.0e-10 7.1e-10 5.7e-10 1.8e-9
    (largest ratio device / f32 restatement: 1.06; the device accumulates in f64, the restatement in f32)"""
    p = prm(max_cg_iter=max_cg, **ASSEMBLY[name])
    r = refs(case, p, ("assembly", name, max_cg))
    if name == "huber_two_steps":
        assert all(r[D]["st"]["huber_branches"]) and all(r[F]["st"]["huber_branches"])
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p)
    assert st.gn_iterations == r[F]["st"]["gn_iterations"] == p.max_gn_iter
    e32 = component_errors(W.to_transforms(r[F]["tf"], F), r[D]["tf"])
    edev = component_errors(T, r[D]["tf"])
    print("\nassembly %s cg=%d  f32 restatement error %s\n  device error %s\n  ratio %s" % (name, max_cg, e32, edev, edev / e32))
    assert (e32 > 0).all() and (edev <= 4 * e32).all(), (edev / e32)
    assert np.abs(T[:, :3, :3] @ T[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-6 and (T[:, 3] == [0, 0, 0, 1]).all()


def test_assembly_past_one_grid_trip():
    """70 000 source points: the per-point kernels stride (256 blocks x 256 lanes = 65 536 lanes per trip).
    First MI355X run: f32 restatement 9.2e-9 1.9e-8 9.8e-9 3.9e-10 6.7e-10 1.3e-9, device 2.8e-10 2.3e-10 9.6e-11 8.2e-11 1.1e-10 3.3e-10"""
    c = W.make_case(n_src=70000, n_dst=2000)
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    p = prm(max_cg_iter=2, w_p2p=0.1)
    f = Field.of(c)
    try:
        T, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], p)
        dense = f.resample(T)
    finally:
        f.close()
    r = {t: W.estimate(c["graph"], t, c["dst"], c["dst_n"], c["src"], c["nn"], p)[0] for t in (F, D)}
    e32, edev = component_errors(W.to_transforms(r[F], F), r[D]), component_errors(T, r[D])
    print("\n70k  f32 %s\n  device %s\n  ratio %s" % (e32, edev, edev / e32))
    assert (edev <= 4 * e32).all(), edev / e32
    want = W.resample(c["graph"], T, F)
    assert np.abs(dense - want).max() < 2e-6


# ---- 2. solve ------------------------------------------------------------------------------------------------------------------------
def test_solve_meets_eigens_promise(case, field):
    """cg_conv_tol = 1e-4, max_cg_iter = 500: |A^T A delta - A^T b| <= c tol |A^T b| in f64 on the restatement's explicit matrices, c = the
    ratio the f32 restatement reaches (through the same f32 read-back) times 2; iterations within +-10 % (at least +-2) of the f32
    restatement's; the reported residual agrees with the recomputed one to twice the f32 restatement's own disagreement.
    First MI355X run: c = 1.59 for the f32 restatement (bound 3.19), 1.12 for the device; iterations 201 (f32), 200 (f64), 201 (device);
    |reported - recomputed| / |A^T b| 7.7e-5 for the f32 restatement, 3.7e-5 for the device."""
    p = prm(cg_conv_tol=1e-4)
    r = refs(case, p, ("solve",))
    At, b, AtA, Atb, _, its32 = r[D]["rec"][0]      # the system at tforms_vec = 0, exact
    its32 = r[F]["rec"][0][5]
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p)
    nb = np.linalg.norm(Atb)

    def ratio(T_):
        return np.linalg.norm(AtA @ readback(T_).reshape(-1) - Atb) / (float(p.cg_conv_tol) * nb)

    c32, cdev = ratio(W.to_transforms(r[F]["tf"], F)), ratio(T)
    rec32 = abs(np.sqrt(r[F]["st"]["last_cg_residual_norm2"]) / nb - c32 * float(p.cg_conv_tol))
    recdev = abs(np.sqrt(st.last_cg_residual_norm2) / nb - cdev * float(p.cg_conv_tol))
    print("\nsolve: c f32 %.4f device %.4f; iterations f32 %d f64 %d device %d; |reported - recomputed| / |Atb|: f32 %.3e device %.3e"
          % (c32, cdev, its32, r[D]["rec"][0][5], st.cg_iterations_total, rec32, recdev))
    assert cdev <= 2 * c32
    assert abs(int(st.cg_iterations_total) - its32) <= max(2, 0.1 * its32)
    assert recdev <= 2 * rec32
    assert st.gn_iterations == 1


# ---- 3. Gauss-Newton -----------------------------------------------------------------------------------------------------------------
def test_gauss_newton(case, field):
    """max_gn_iter = 5: converged and gn_iterations as the f32 restatement's; the final unknowns within the step-1 tolerance times the
    number of steps.  First MI355X run: 2 steps, converged; step-1 tolerance 4.6e-7 2.3e-7 1.7e-7 2.4e-7 6.6e-8 3.2e-7 (4 x the f32
    restatement's error after one full step: its CG stops one iteration apart from the f64 one's); device error 1.1e-9 3.1e-9 7.6e-9
    4.1e-9 9.5e-10 1.3e-9."""
    p5, p1 = prm(max_gn_iter=5), prm(max_gn_iter=1)
    r5, r1 = refs(case, p5, ("gn", 5)), refs(case, p1, ("gn", 1))
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p5)
    assert (st.gn_iterations, bool(st.converged)) == (r5[F]["st"]["gn_iterations"], r5[F]["st"]["converged"])
    step1 = 4 * component_errors(W.to_transforms(r1[F]["tf"], F), r1[D]["tf"])
    edev = component_errors(T, r5[D]["tf"])
    print("\ngn: iterations %d converged %d; step-1 tolerance %s; device error %s" % (st.gn_iterations, st.converged, step1, edev))
    assert (edev <= st.gn_iterations * step1).all()
    assert st.max_delta_sq == pytest.approx(r5[F]["st"]["max_delta_sq"], rel=1e-2)


# ---- 4. utilities --------------------------------------------------------------------------------------------------------------------
def test_transform_points_per_point_is_bit_exact(case):
    rng = np.random.RandomState(1)
    n = 70001
    tf = rng.standard_normal((n, 6)) * [0.3, 0.3, 0.3, 0.1, 0.1, 0.1]
    T = W.to_transforms(tf.reshape(-1), F)
    xyz = rng.standard_normal((n, 3)).astype(F)
    assert transform_points(T, xyz).tobytes() == W.transform_points(T, xyz).tobytes()


def test_resample(case, field):
    """against the f32 restatement to the polish's tolerance: the f32 SVD polish measured against the f64 polish of the same f32 blend.
    First MI355X run: f32 restatement against f64 1.2e-7, device against f64 3.0e-8 (the device polishes in f64 and rounds once)."""
    tf = np.random.RandomState(2).standard_normal((case["n_ctrl"], 6)) * [0.05, 0.05, 0.05, 0.01, 0.01, 0.01]
    T = W.to_transforms(tf.reshape(-1), F)
    got, want32, want64 = field.resample(T), W.resample(case["graph"], T, F), W.resample(case["graph"], T, D)
    tol = 4 * np.abs(want32.astype(D) - want64).max()
    print("\nresample: f32 restatement vs f64 %.3e, device vs f64 %.3e" % (tol / 4, np.abs(got - want64).max()))
    assert np.abs(got - want64).max() <= tol
    assert (got[:, 3] == [0, 0, 0, 1]).all()


def test_resample_gives_the_identity_where_every_weight_underflows(case):
    c = dict(case, ctrl_sigma=F(1e-4))
    g = W.Graph(c["n_ctrl"], c["ctrl_idx"], c["ctrl_d2"], W.RBF, c["ctrl_sigma"], c["reg_idx"], c["reg_d2"], W.RBF, c["reg_sigma"])
    dead = g.total == 0
    assert dead.sum() > 100 and (~dead).sum() >= 0
    f = Field.of(c)
    try:
        T = W.to_transforms((np.random.RandomState(3).standard_normal((c["n_ctrl"], 6)) * 0.05).reshape(-1), F)
        got = f.resample(T)
        assert (got[dead] == np.eye(4, dtype=F)).all()
        assert np.abs(got[~dead] - W.resample(g, T, F)[~dead]).max() < 2e-6 if (~dead).any() else True
        # and the estimator gives such points rows of zeros (:1687-1690): finite output
        Te, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm())
        assert np.isfinite(Te).all()
    finally:
        f.close()


# ---- 5. the loop, 6. reproducibility ------------------------------------------------------------------------------------------------
def icp_run(case, field, p, max_iter, conv_tol=2.5e-3, ctx=None):
    from cilantro_amd.icp import Context

    own = ctx is None
    ctx = Context(0) if own else ctx
    try:
        if own:
            ctx.set_target(case["dst"], case["dst_n"])
            ctx.set_source(case["src"])
        ctrl, dense, res = np.zeros(16 * case["n_ctrl"], F), np.zeros(16 * len(case["src"]), F), capi.IcpResult()
        rc = ctx._L.cilhip_warp_field_icp_run(ctx._h, field.h, C.byref(cparams(p)), max_iter, conv_tol, float(case["max_sq"]), None, ctrl.ctypes.data, dense.ctypes.data, C.byref(res))
        assert rc == capi.OK, ctx._L.cilhip_last_error(ctx._h)
        return dict(T=ctrl.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), dense=dense.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), iterations=int(res.iterations),
                    last_delta_norm=float(res.last_delta_norm), ncorr=int(res.last_ncorr), bytes=ctrl.tobytes() + dense.tobytes())
    finally:
        if own:
            ctx.close()


def test_icp_loop(case, field):
    """the example's parameters on the synthetic pair: the warped source's mean point-to-plane residual falls below the best rigid
    alignment's by at least the factor the f32 restatement's loop reaches, less 10 %.
    First MI355X run: rigid 1.784e-3, restatement 1.026e-3 (factor 1.739), device 1.026e-3 (factor 1.739); 2 iterations each; 3 000
    correspondences in every iteration of both (the threshold band is empty on this pair)."""
    from cilantro_amd.icp import SimpleCombinedMetricRigidICP3f

    p = prm()
    ref = W.icp_loop(case["graph"], F, case["dst"], case["dst_n"], case["src"], p, 15, 2.5e-3, case["max_sq"])
    got = icp_run(case, field, p, 15)
    rigid = SimpleCombinedMetricRigidICP3f(case["dst"], case["dst_n"], case["src"])
    rigid.correspondenceSearchEngine().setMaxDistance(case["max_sq"])
    rigid.setMaxNumberOfIterations(30).setConvergenceTolerance(1e-6)
    Tr = rigid.estimate().getTransform().astype(D)
    rigid_res = W.plane_residuals(case["dst"], case["dst_n"], case["src"].astype(D) @ Tr[:3, :3].T + Tr[:3, 3]).mean()
    warped = transform_points(got["dense"], case["src"])
    res_dev, res_ref = W.plane_residuals(case["dst"], case["dst_n"], warped).mean(), W.plane_residuals(case["dst"], case["dst_n"], ref["warped"]).mean()
    print("\nloop: rigid %.3e, restatement %.3e (factor %.3f), device %.3e (factor %.3f); iterations %d / %d; ncorr %s / %d"
          % (rigid_res, res_ref, rigid_res / res_ref, res_dev, rigid_res / res_dev, ref["iterations"], got["iterations"], ref["ncorr"], got["ncorr"]))
    assert rigid_res / res_ref > 1.0
    assert rigid_res / res_dev >= 0.9 * (rigid_res / res_ref)
    assert got["iterations"] == ref["iterations"]
    # correspondence counts: equal in the first two iterations
    for k in (1, 2):
        if k <= len(ref["ncorr"]):
            assert icp_run(case, field, p, k, conv_tol=0.0)["ncorr"] == ref["ncorr"][k - 1]
    # afterwards they may differ by the points whose nearest-neighbour distance lies within 1e-5 of the threshold (positions are O(1):
    # f32 transforms that agree to ~1e-6 move a point by less than that); the restatement finds at most 1 % of the source there
    d = np.sqrt(W.d2_pinned(ref["warped"], case["dst"]).min(1).astype(D))
    band = int((np.abs(d - np.sqrt(float(case["max_sq"]))) < 1e-5).sum())
    assert band <= 0.01 * len(case["src"])
    assert abs(got["ncorr"] - ref["ncorr"][-1]) <= band


def test_icp_loop_leaves_the_context_with_the_callers_source(case, field):
    from cilantro_amd.icp import Context

    ctx = Context(0)
    try:
        ctx.set_target(case["dst"], case["dst_n"])
        ctx.set_source(case["src"])
        before = ctx.compute_residuals(capi.METRIC_COMBINED, 0.0, 1.0, np.eye(4, dtype=F)).tobytes()
        icp_run(case, field, prm(), 2, ctx=ctx)
        assert ctx.compute_residuals(capi.METRIC_COMBINED, 0.0, 1.0, np.eye(4, dtype=F)).tobytes() == before
    finally:
        ctx.close()


def test_two_runs_give_the_same_bytes(case, field):
    p = prm(cg_conv_tol=1e-4)
    a, b = (field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p) for _ in range(2))
    assert a[2] == b[2] and bytes(a[1]) == bytes(b[1])
    f2 = Field.of(case)
    try:
        assert icp_run(case, field, prm(), 3)["bytes"] == icp_run(case, f2, prm(), 3)["bytes"]
    finally:
        f2.close()


# ---- 7. the dense mirror -------------------------------------------------------------------------------------------------------------
def test_dense_mirror():
    """400 points, every point its own control node (ctrl_idx[i] = i, k_ctrl = 1, Unity), k_reg = 6: the restatement's dense system.
    First MI355X run: f32 restatement 3.5e-8 2.5e-8 1.4e-8 2.8e-11 2.7e-11 4.8e-11, device 1.9e-11 1.3e-11 1.5e-11 1.1e-11 1.7e-11 1.9e-11"""
    from cilantro_amd import synthetic

    src, _ = synthetic.make_surface(400, seed=45)
    flat, nrm = synthetic.make_surface(600, seed=46)
    dst = synthetic.bend(flat)
    reg_idx, reg_d2 = W.knn_lists(src, src, 6)
    own, zero, sigma = np.arange(400, dtype=np.uint32)[:, None], np.zeros((400, 1), F), F(0.2)
    g = W.Graph(400, own, zero, W.UNITY, 1.0, reg_idx, reg_d2, W.RBF, sigma)
    nn = W.nearest(dst, src, F(0.1 ** 2))
    p = prm(w_p2p=0.1, max_cg_iter=2)
    # the sparse restatement IS the dense estimator's system on these lists (tests/test_warp_refs_cpu.py pins it); here once more at step 0
    At, b, _ = W.assemble(g, D, dst, nrm, src, nn, np.zeros(2400), p)
    A, bd = W.assemble_dense_literal(D, dst, nrm, src, nn, reg_idx, np.sqrt(W.eval_weights(W.RBF, sigma, reg_d2)), np.zeros(2400), p)
    assert np.abs(At.T.toarray() - A).max() <= 1e-14 * np.abs(A).max() and np.abs(b - bd).max() <= 1e-14 * np.abs(bd).max()
    f = Field(400, 400, own, zero, W.UNITY, 1.0, reg_idx, reg_d2, W.RBF, sigma)
    try:
        T, st, _ = f.estimate(dst, nrm, src, nn, p)
    finally:
        f.close()
    r = {t: W.estimate(g, t, dst, nrm, src, nn, p)[0] for t in (F, D)}
    e32, edev = component_errors(W.to_transforms(r[F], F), r[D]), component_errors(T, r[D])
    print("\ndense: f32 %s\n  device %s" % (e32, edev))
    assert (edev <= 4 * e32).all(), edev / e32


def test_dense_python_mirror_runs():
    from cilantro_amd import synthetic
    from cilantro_amd.icp import SimpleCombinedMetricDenseRigidWarpFieldICP3f

    src, _ = synthetic.make_surface(400, seed=45)
    flat, nrm = synthetic.make_surface(600, seed=46)
    dst = synthetic.bend(flat)
    icp = SimpleCombinedMetricDenseRigidWarpFieldICP3f(dst, nrm, src, W.knn_lists(src, src, 6))
    icp.correspondenceSearchEngine().setMaxDistance(0.1 ** 2)
    icp.regularizationWeightEvaluator().setSigma(0.2)
    icp.setMaxNumberOfIterations(3).setConvergenceTolerance(2.5e-3).setMaxNumberOfGaussNewtonIterations(1).setStiffnessRegularizationWeight(200.0).setHuberLossBoundary(1e-2)
    icp.setPointToPointMetricWeight(0.1)
    T = icp.estimate().getTransform()
    assert T.shape == (400, 4, 4) and np.isfinite(T).all() and 1 <= icp.getNumberOfPerformedIterations() <= 3
    before = W.plane_residuals(dst, nrm, src).mean()
    res = icp.getResiduals()
    assert res.shape == (400,) and np.isfinite(res).all()
    from cilantro_amd.icp import transformPoints

    assert W.plane_residuals(dst, nrm, transformPoints(icp.getDenseWarpField(), src)).mean() < before


# ---- 8. degenerate inputs, and the rules that need a handle -----------------------------------------------------------------------
def test_no_matches_give_the_identity_and_no_convergence(case, field):
    none = np.full(len(case["src"]), W.NONE, np.uint32)
    for nn, p in ((none, prm()), (case["nn"], prm(w_p2p=0.0, w_p2pl=0.0))):
        T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], nn, p)
        assert (T == np.eye(4, dtype=F)).all() and (st.gn_iterations, st.converged, st.cg_iterations_total) == (0, 0, 0)
    got = icp_run(dict(case, max_sq=F(1e-12)), field, prm(), 3)
    assert (got["T"] == np.eye(4, dtype=F)).all() and got["ncorr"] == 0 and got["iterations"] == 1 and got["last_delta_norm"] == 0.0


def test_a_node_no_source_point_names(case):
    """such a node moves through regularisation only and stays finite; with w_reg = 0 its diagonal is 0, M^-1 = 1 and its delta stays 0"""
    lonely = int(case["ctrl_idx"][0, 0])
    idx = case["ctrl_idx"].copy()
    idx[idx == lonely] = W.NONE
    c = dict(case, ctrl_idx=idx)
    g = W.Graph(c["n_ctrl"], idx, c["ctrl_d2"], c["ctrl_kernel"], c["ctrl_sigma"], c["reg_idx"], c["reg_d2"], c["reg_kernel"], c["reg_sigma"])
    f = Field.of(c)
    try:
        T, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm())
        want = W.estimate(g, D, c["dst"], c["dst_n"], c["src"], c["nn"], prm())[0].reshape(-1, 6)
        assert np.isfinite(T).all() and np.abs(want[lonely]).max() > 0
        assert np.abs(readback(T)[lonely]).max() > 0.25 * np.abs(want[lonely]).max()
        T0, st0, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm(w_reg=0.0))
        assert np.isfinite(T0).all() and (T0[lonely] == np.eye(4, dtype=F)).all()
    finally:
        f.close()


def test_rules_that_need_a_handle(case, field):
    args = (case["dst"], case["dst_n"], case["src"], case["nn"])
    for bad in (dict(w_p2pl=float("nan")), dict(w_reg=-1.0), dict(huber_boundary=0.0), dict(gn_conv_tol=float("inf")), dict(cg_conv_tol=float("nan")), dict(w_p2p=float("inf"))):
        T, st, _ = field.estimate(*args, prm(**bad), expect=capi.ERR_INVALID)
        assert (T == 7).all() and "warp_field_estimate" in last_error(field.L)
    T, _, _ = field.estimate(case["dst"], None, case["src"], case["nn"], prm(), expect=capi.ERR_INVALID)
    assert (T == 7).all()
    from cilantro_amd.icp import Context

    ctx = Context(0)
    try:
        ctrl, res = np.full(16 * case["n_ctrl"], 7, F), capi.IcpResult()

        def run():
            return ctx._L.cilhip_warp_field_icp_run(ctx._h, field.h, C.byref(cparams(prm())), 2, 1e-3, float(case["max_sq"]), None, ctrl.ctypes.data, None, C.byref(res))

        assert run() == capi.ERR_INVALID      # no target, no source
        ctx.set_target(case["dst"], None)
        ctx.set_source(case["src"])
        assert run() == capi.ERR_INVALID and b"normals" in ctx._L.cilhip_last_error(ctx._h)      # w_p2pl > 0
        ctx.set_target(case["dst"], case["dst_n"])
        ctx.set_source(case["src"][:100])
        assert run() == capi.ERR_INVALID      # another size than the field's
        ctx.set_source(case["src"])
        ctx.set_option("search_direction", 1)
        assert run() == capi.ERR_UNSUPPORTED
        ctx.set_option("search_direction", 0)
        ctx.set_projection(np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], F), 640, 480)
        assert run() == capi.ERR_UNSUPPORTED and b"projection" in ctx._L.cilhip_last_error(ctx._h)
        ctx.set_projection(None)
        assert (ctrl == 7).all()
        assert run() == capi.OK
    finally:
        ctx.close()
    # device-resident lists with a bad index are refused after the device is opened
    import torch

    bad = case["ctrl_idx"].copy()
    bad[5, 1] = case["n_ctrl"]
    L, h = capi.load(), C.c_void_p()
    t = [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda() for a in (bad, case["ctrl_d2"], case["reg_idx"], case["reg_d2"])]
    torch.cuda.synchronize()
    rc = L.cilhip_warp_field_create(0, len(case["src"]), case["n_ctrl"], t[0].data_ptr(), t[1].data_ptr(), 4, 1, 0.035, t[2].data_ptr(), t[3].data_ptr(), 8, 1, 0.21, capi.MEM_DEVICE, C.byref(h))
    assert rc == capi.ERR_INVALID and not h.value and "n_ctrl" in last_error(L)
