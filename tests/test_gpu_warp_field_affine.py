"""GPU: the affine warp-field entries of c_api.h against tests/_warp_affine_refs.py, through the C ABI.

Yardsticks, as in tests/test_gpu_warp_field.py: the f64 restatement is "the exact answer", the f32 restatement "the reference as it
runs"; unless a test says otherwise a tolerance is the f32 restatement's own error against the f64 one on the same inputs, times 4
(slack for a different but equally valid summation order), per component class -- the linear 9 and the translation 3, the maximum over
the control nodes -- read straight from the returned matrices (the f32 restatement goes through the same f32 matrices first).

Shapes: _warp_refs.make_case(): 3 000 source / 4 000 target points, 286 control nodes (not a multiple of 64, more than one block of
nodes, ragged lists at the border), 2 002 arcs, k_ctrl = 4, k_reg = 8; one case with 70 000 source points (more than one grid trip of
the per-point kernels).  w_reg = 1 and max_cg_iter = 1000 wherever CG runs freely: at the example's w_reg = 200 the affine system is so
ill-conditioned that the f32 and f64 restatements end 4e-3 apart (section 17.4), and no tolerance follows from that.

The pin of A3's s_t: two Gauss-Newton steps of 1 or 2 CG iterations at huber_boundary = 2e-5.  The second linearisation is the first
at which s_t != s, and it meets both Huber branches.  An f64 restatement that puts s into the rows (the "corrected" Jacobian) lies
more than 8 times the f32 restatement's error away from the f64 restatement, so the 4 x bound tells the two apart.

Figures of the first MI355X run are recorded in the docstrings of the tests that measure them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _warp_affine_refs as A
import _warp_refs as W
from cilantro_amd import capi
from test_gpu_warp_field import Field, cparams, last_error, transform_points

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
HOST = capi.MEM_HOST
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class AffineField(Field):
    """the same handle; estimate / resample go through the affine entries (`rigid=True`: the rigid ones, for the shared-scratch test)"""

    def estimate(self, dst, nrm, src, nn, p, expect=capi.OK, rigid=False):
        if rigid:
            return Field.estimate(self, dst, nrm, src, nn, p, expect)
        dst, src, nn = np.ascontiguousarray(dst, F), np.ascontiguousarray(src, F), np.ascontiguousarray(nn, np.uint32)
        nrm = None if nrm is None else np.ascontiguousarray(nrm, F)
        out, st = np.full(16 * self.n_ctrl, 7, F), capi.WarpStats()
        rc = self.L.cilhip_warp_field_estimate_affine3f(self.h, dst.ctypes.data, None if nrm is None else nrm.ctypes.data, len(dst), src.ctypes.data, nn.ctypes.data, HOST,
                                                        C.byref(cparams(p)), out.ctypes.data, C.byref(st))
        assert rc == expect, last_error(self.L)
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), st, out.tobytes()

    def resample(self, T):
        t = np.ascontiguousarray(np.asarray(T, F).transpose(0, 2, 1)).reshape(-1)
        out = np.zeros(16 * self.n_src, F)
        assert self.L.cilhip_warp_field_resample_affine3f(self.h, t.ctypes.data, out.ctypes.data, HOST) == capi.OK, last_error(self.L)
        return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()


def prm(**kw):
    """the example's parameters (examples/non_rigid_icp.cpp:75-82) with the stiffness and the CG cap the affine system needs"""
    base = dict(w_p2p=0.0, w_p2pl=1.0, w_reg=1.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=1000, cg_conv_tol=1e-5)
    base.update(kw)
    return W.Params(**base)


def class_errors(T_or_tf, exact_tf):
    """(linear 9, translation 3): the maximum over the nodes of |read-back - exact|, f64"""
    got = A.readback(T_or_tf) if np.ndim(T_or_tf) == 3 else np.asarray(T_or_tf, D).reshape(-1, 12)
    d = np.abs(got - np.asarray(exact_tf, D).reshape(-1, 12))
    return np.array([d[:, :9].max(), d[:, 9:].max()])


@pytest.fixture(scope="module")
def case():
    c = W.make_case()
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    assert 150 <= c["n_ctrl"] <= 300 and c["n_ctrl"] % 64 != 0
    assert (c["nn"] != W.NONE).sum() > 2000
    return c


@pytest.fixture(scope="module")
def field(case):
    f = AffineField.of(case)
    yield f
    f.close()


_REFS = {}


def refs(case, p, key):
    """the f32 and f64 restatements of one estimate, computed once per parameter set"""
    if key not in _REFS:
        out = {}
        for t in (F, D):
            rec = []
            tf, st = A.estimate(case["graph"], t, case["dst"], case["dst_n"], case["src"], case["nn"], p, record=rec)
            out[t] = dict(tf=tf, st=st, rec=rec)
        _REFS[key] = out
    return _REFS[key]


PIN = dict(huber_boundary=2e-5, max_gn_iter=2, gn_conv_tol=0.0)
ASSEMBLY = {"plane": dict(), "point_and_plane": dict(w_p2p=0.1), "pin_plane": dict(PIN), "pin_point_and_plane": dict(PIN, w_p2p=0.1)}


# ---- 1. assembly, isolated from convergence; the pin of s_t -----------------------------------------------------------------------
@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("name", list(ASSEMBLY))
def test_assembly_after_one_and_two_cg_iterations(case, field, name, max_cg):
    """x1 = alpha M^-1 A^T b exercises A^T b, the diagonal and one operator application; x2 one more.  The pin cases run two steps: the
    second linearisation has s_t != s and both Huber branches.
    Errors against the f64 restatement per class (linear, translation): f32 restatement / f64 restatement with s in the rows:
      plane, 1 CG iteration        6.0e-8 5.4e-9      plane, 2                 6.0e-8 5.9e-9
      point and plane, 1           6.0e-8 4.9e-9      point and plane, 2       6.3e-8 5.3e-9
      pin plane, 1                 7.3e-7 1.2e-8  /  2.6e-5 8.1e-7      pin plane, 2             2.3e-7 1.5e-8  /  1.2e-5 1.4e-6
      pin point and plane, 1       7.1e-7 1.5e-8  /  3.2e-5 7.3e-7      pin point and plane, 2   6.6e-7 3.8e-8  /  2.0e-5 1.5e-6
    (the linear figure of the one-step cases is half an ulp of the stored 1 + x)
    First MI355X run, device error (linear, translation):
      plane, 1                     6.0e-8 6.0e-9      plane, 2                 6.0e-8 6.0e-9
      point and plane, 1           6.0e-8 5.4e-9      point and plane, 2       5.9e-8 5.8e-9
      pin plane, 1                 7.3e-7 1.0e-8      pin plane, 2             2.3e-7 1.4e-8
      pin point and plane, 1       7.1e-7 1.3e-8      pin point and plane, 2   6.6e-7 3.6e-8
    (largest ratio device / f32 restatement 1.11; in the linear class the two errors are the same number to nine digits in seven of the
    eight cases: the rounding of the stored 1 + x.  The s-variant lies 31 to 52 times the f32 error away in the linear class and 40 to
    93 times in the translations.)"""
    p = prm(max_cg_iter=max_cg, **ASSEMBLY[name])
    r = refs(case, p, ("assembly", name, max_cg))
    e32 = class_errors(A.to_transforms(r[F]["tf"], F), r[D]["tf"])
    if name.startswith("pin"):
        assert all(r[D]["st"]["huber_branches"]) and all(r[F]["st"]["huber_branches"])
        tf_s, _ = A.estimate(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], p, jac_point="s")
        es = class_errors(tf_s, r[D]["tf"])
        print("\n  the s-variant lies %s x the f32 error away" % (es / e32))
        assert (es > 8 * e32).all(), es / e32
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p)
    assert st.gn_iterations == r[F]["st"]["gn_iterations"] == p.max_gn_iter
    edev = class_errors(T, r[D]["tf"])
    print("\nassembly %s cg=%d  f32 restatement error %s\n  device error %s\n  ratio %s" % (name, max_cg, e32, edev, edev / e32))
    assert (e32 > 0).all() and (edev <= 4 * e32).all(), (edev / e32)
    assert (T[:, 3] == [0, 0, 0, 1]).all()


def test_assembly_past_one_grid_trip():
    """70 000 source points: the per-point kernels stride (256 blocks x 256 lanes = 65 536 lanes per trip).
    First MI355X run: f32 restatement 6.2e-8 6.3e-9, device 6.2e-8 4.9e-9; the resample equals the f32 restatement's"""
    c = W.make_case(n_src=70000, n_dst=2000)
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    p = prm(max_cg_iter=2, w_p2p=0.1)
    f = AffineField.of(c)
    try:
        T, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], p)
        dense = f.resample(T)
    finally:
        f.close()
    r = {t: A.estimate(c["graph"], t, c["dst"], c["dst_n"], c["src"], c["nn"], p)[0] for t in (F, D)}
    e32, edev = class_errors(A.to_transforms(r[F], F), r[D]), class_errors(T, r[D])
    print("\n70k  f32 %s\n  device %s\n  ratio %s" % (e32, edev, edev / e32))
    assert (edev <= 4 * e32).all(), edev / e32
    assert np.abs(dense - A.resample(c["graph"], T, F)).max() < 2e-6


# ---- 2. solve ------------------------------------------------------------------------------------------------------------------------
def test_solve_meets_eigens_promise(case, field):
    """cg_conv_tol = 1e-4, one step: |A^T A delta - A^T b| <= c tol |A^T b| in f64 on the restatement's explicit matrices, c = the ratio
    the f32 restatement reaches (through the same f32 read-back) times 2; cg_iterations_total within 10 % of the band the two
    restatements span (the device accumulates in f64 and stores in f32: it may land anywhere between them); the reported residual
    agrees with the recomputed one to twice the f32 restatement's own disagreement.
    Restatements: 396 iterations (f32), 373 (f64).  First MI355X run: 395 iterations; c = 0.903 for the f32 restatement (bound 1.81),
    0.833 for the device; |reported - recomputed| / |A^T b| 1.0e-6 for the f32 restatement, 5.3e-7 for the device."""
    p = prm(cg_conv_tol=1e-4)
    r = refs(case, p, ("solve",))
    At, b, AtA, Atb, _, its64 = r[D]["rec"][0]      # the system at the start, exact
    its32 = r[F]["rec"][0][5]
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p)
    nb = np.linalg.norm(Atb)
    start = A.identity_start(case["n_ctrl"], D)

    def ratio(T_):
        return np.linalg.norm(AtA @ (A.readback(T_).reshape(-1) - start) - Atb) / (float(p.cg_conv_tol) * nb)

    c32, cdev = ratio(A.to_transforms(r[F]["tf"], F)), ratio(T)
    rec32 = abs(np.sqrt(r[F]["st"]["last_cg_residual_norm2"]) / nb - c32 * float(p.cg_conv_tol))
    recdev = abs(np.sqrt(st.last_cg_residual_norm2) / nb - cdev * float(p.cg_conv_tol))
    print("\nsolve: c f32 %.4f device %.4f; iterations f32 %d f64 %d device %d; |reported - recomputed| / |Atb|: f32 %.3e device %.3e"
          % (c32, cdev, its32, its64, st.cg_iterations_total, rec32, recdev))
    assert cdev <= 2 * c32
    assert 0.9 * min(its32, its64) <= int(st.cg_iterations_total) <= 1.1 * max(its32, its64)
    assert recdev <= 2 * rec32
    assert st.gn_iterations == 1


# ---- 3. Gauss-Newton -----------------------------------------------------------------------------------------------------------------
def test_gauss_newton(case, field):
    """max_gn_iter = 5: converged and gn_iterations as the f32 restatement's (the two restatements agree: 3 steps, converged; CG
    iterations 500 / 658 / 455 in f32, 436 / 516 / 393 in f64); the final unknowns within the one-full-step tolerance times the number
    of steps; max_delta_sq within 1e-2 relative.
    First MI355X run: 3 steps, converged, 1 559 CG iterations in all (f32 restatement 1 613, f64 1 345); one-full-step tolerance 2.9e-5
    2.9e-6 (4 x the f32 restatement's error after one step: its CG stops 64 iterations after the f64 one's); device error 1.0e-7 2.0e-8;
    max_delta_sq 3.2129e-10 against the f32 restatement's 3.1851e-10 (0.87 %)."""
    p5, p1 = prm(max_gn_iter=5), prm(max_gn_iter=1)
    r5, r1 = refs(case, p5, ("gn", 5)), refs(case, p1, ("gn", 1))
    assert (r5[F]["st"]["gn_iterations"], r5[F]["st"]["converged"]) == (r5[D]["st"]["gn_iterations"], r5[D]["st"]["converged"]) == (3, True)
    T, st, _ = field.estimate(case["dst"], case["dst_n"], case["src"], case["nn"], p5)
    step1 = 4 * class_errors(A.to_transforms(r1[F]["tf"], F), r1[D]["tf"])
    edev = class_errors(T, r5[D]["tf"])
    print("\ngn: iterations %d converged %d cg %d; step-1 tolerance %s; device error %s; max_delta_sq %.6e (f32 %.6e)"
          % (st.gn_iterations, st.converged, st.cg_iterations_total, step1, edev, st.max_delta_sq, r5[F]["st"]["max_delta_sq"]))
    assert (st.gn_iterations, bool(st.converged)) == (r5[F]["st"]["gn_iterations"], r5[F]["st"]["converged"])
    assert (edev <= st.gn_iterations * step1).all()
    assert st.max_delta_sq == pytest.approx(r5[F]["st"]["max_delta_sq"], rel=1e-2)


# ---- 4. utilities --------------------------------------------------------------------------------------------------------------------
def random_affine(n, seed):
    T = np.tile(np.eye(4), (n, 1, 1))
    T[:, :3, :] += np.random.RandomState(seed).standard_normal((n, 3, 4)) * 0.1
    return T.astype(F)


def test_resample(case, field):
    """random affine control transforms (far from rotations: a polish would show) against the f64 restatement.
    First MI355X run: f32 restatement against f64 2.3e-7, device against f64 2.3e-7 (the same f32 operations in the same order)."""
    T = random_affine(case["n_ctrl"], 2)
    got, want32, want64 = field.resample(T), A.resample(case["graph"], T, F), A.resample(case["graph"], T, D)
    tol = 4 * np.abs(want32.astype(D) - want64).max()
    print("\nresample: f32 restatement vs f64 %.3e, device vs f64 %.3e" % (tol / 4, np.abs(got - want64).max()))
    assert tol > 0 and np.abs(got - want64).max() <= tol
    assert (got[:, 3] == [0, 0, 0, 1]).all()
    assert np.abs(got[:, :3, :3] @ got[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() > 1e-2      # (no polish)


def test_resample_gives_the_identity_where_every_weight_underflows(case):
    c = dict(case, ctrl_sigma=F(1e-4))
    g = W.Graph(c["n_ctrl"], c["ctrl_idx"], c["ctrl_d2"], W.RBF, c["ctrl_sigma"], c["reg_idx"], c["reg_d2"], W.RBF, c["reg_sigma"])
    dead = g.total == 0
    assert dead.sum() > 100
    f = AffineField.of(c)
    try:
        T = random_affine(c["n_ctrl"], 3)
        got = f.resample(T)
        assert got[dead].tobytes() == np.tile(np.eye(4, dtype=F), (int(dead.sum()), 1, 1)).tobytes()
        if (~dead).any():
            assert np.abs(got[~dead] - A.resample(g, T, F)[~dead]).max() < 2e-6
        Te, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm())      # such points give rows of zeros (:2068-2071)
        assert np.isfinite(Te).all()
    finally:
        f.close()


# ---- 5. the loop, 6. reproducibility ------------------------------------------------------------------------------------------------
def icp_run(case, field, p, max_iter, conv_tol=2.5e-3, ctx=None, rigid=False):
    from cilantro_amd.icp import Context

    own = ctx is None
    ctx = Context(0) if own else ctx
    try:
        if own:
            ctx.set_target(case["dst"], case["dst_n"])
            ctx.set_source(case["src"])
        ctrl, dense, res = np.zeros(16 * case["n_ctrl"], F), np.zeros(16 * len(case["src"]), F), capi.IcpResult()
        entry = ctx._L.cilhip_warp_field_icp_run if rigid else ctx._L.cilhip_warp_field_icp_run_affine
        rc = entry(ctx._h, field.h, C.byref(cparams(p)), max_iter, conv_tol, float(case["max_sq"]), None, ctrl.ctypes.data, dense.ctypes.data, C.byref(res))
        assert rc == capi.OK, ctx._L.cilhip_last_error(ctx._h)
        return dict(T=ctrl.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), dense=dense.reshape(-1, 4, 4).transpose(0, 2, 1).copy(), iterations=int(res.iterations),
                    last_delta_norm=float(res.last_delta_norm), ncorr=int(res.last_ncorr), bytes=ctrl.tobytes() + dense.tobytes())
    finally:
        if own:
            ctx.close()


def test_icp_loop(case, field):
    """15 iterations of one Gauss-Newton step each: the warped source's mean point-to-plane residual falls below the best rigid
    alignment's by at least the factor the f32 restatement's loop reaches, less 10 %.
    First MI355X run: rigid 1.784e-3, restatement 9.18e-5 (factor 19.4), device 9.18e-5 (factor 19.4); 2 iterations each; 3 000
    correspondences in every iteration of both (the threshold band is empty on this pair)."""
    from cilantro_amd.icp import SimpleCombinedMetricRigidICP3f

    p = prm()
    ref = A.icp_loop(case["graph"], F, case["dst"], case["dst_n"], case["src"], p, 15, 2.5e-3, case["max_sq"])
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
    for k in (1, 2):      # correspondence counts: equal in the first two iterations
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


def test_two_runs_give_the_same_bytes_and_the_grown_scratch_changes_nothing(case):
    """two estimates and two loops on two handles; a rigid estimate on one handle before and after its first affine one"""
    p = prm(cg_conv_tol=1e-4)
    args = (case["dst"], case["dst_n"], case["src"], case["nn"])
    f1, f2 = AffineField.of(case), AffineField.of(case)
    try:
        rigid_p = prm(w_reg=200.0, max_cg_iter=500)
        rigid_before = f1.estimate(*args, rigid_p, rigid=True)
        a, b = f1.estimate(*args, p), f2.estimate(*args, p)
        assert a[2] == b[2] and bytes(a[1]) == bytes(b[1])
        rigid_after = f1.estimate(*args, rigid_p, rigid=True)
        assert rigid_before[2] == rigid_after[2] and bytes(rigid_before[1]) == bytes(rigid_after[1])
        assert not (rigid_before[0] == np.eye(4, dtype=F)).all() and rigid_before[2] != a[2]
        assert icp_run(case, f1, prm(), 3)["bytes"] == icp_run(case, f2, prm(), 3)["bytes"]
        f3 = AffineField.of(case)      # (never ran an affine call: its scratch has the size of its creation)
        try:
            assert icp_run(case, f1, rigid_p, 2, rigid=True)["bytes"] == icp_run(case, f3, rigid_p, 2, rigid=True)["bytes"]
        finally:
            f3.close()
    finally:
        f1.close(); f2.close()


# ---- 7. degenerate inputs, and the rules that need a handle -----------------------------------------------------------------------
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
    f = AffineField.of(c)
    try:
        T, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm())
        assert np.isfinite(T).all() and not (T[lonely] == np.eye(4, dtype=F)).all()
        T0, st0, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], prm(w_reg=0.0))
        assert np.isfinite(T0).all() and (T0[lonely] == np.eye(4, dtype=F)).all()
    finally:
        f.close()


def test_rules_that_need_a_handle(case, field):
    args = (case["dst"], case["dst_n"], case["src"], case["nn"])
    for bad in (dict(w_p2pl=float("nan")), dict(w_reg=-1.0), dict(huber_boundary=0.0), dict(gn_conv_tol=float("inf")), dict(cg_conv_tol=float("nan")), dict(w_p2p=float("inf"))):
        T, st, _ = field.estimate(*args, prm(**bad), expect=capi.ERR_INVALID)
        assert (T == 7).all() and "warp_field_estimate_affine" in last_error(field.L)
    T, _, _ = field.estimate(case["dst"], None, case["src"], case["nn"], prm(), expect=capi.ERR_INVALID)
    assert (T == 7).all()
    from cilantro_amd.icp import Context

    ctx = Context(0)
    try:
        ctrl, res = np.full(16 * case["n_ctrl"], 7, F), capi.IcpResult()

        def run(p=prm(), handle=field.h, tol=1e-3):
            return ctx._L.cilhip_warp_field_icp_run_affine(ctx._h, handle, C.byref(cparams(p)), 2, tol, float(case["max_sq"]), None, ctrl.ctypes.data, None, C.byref(res))

        def why():
            return ctx._L.cilhip_last_error(ctx._h)

        assert run() == capi.ERR_INVALID and b"warp_field_icp_run_affine" in why()      # no target, no source
        # a NULL field, a bad parameter and a non-finite tolerance come first, as in the rigid loop
        assert run(handle=None) == capi.ERR_INVALID and b"null" in why()
        assert run(p=prm(huber_boundary=0.0)) == capi.ERR_INVALID and b"huber_boundary" in why()
        assert run(p=prm(w_reg=-1.0)) == capi.ERR_INVALID and run(tol=float("nan")) == capi.ERR_INVALID
        ctx.set_target(case["dst"], None)
        ctx.set_source(case["src"])
        assert run() == capi.ERR_INVALID and b"normals" in why()      # w_p2pl > 0
        ctx.set_target(case["dst"], case["dst_n"])
        ctx.set_source(case["src"][:100])
        assert run() == capi.ERR_INVALID      # another size than the field's
        ctx.set_source(case["src"])
        ctx.set_option("search_direction", 1)
        assert run() == capi.ERR_UNSUPPORTED and b"direction" in why()
        ctx.set_option("search_direction", 0)
        ctx.set_projection(np.array([[500, 0, 320], [0, 500, 240], [0, 0, 1]], F), 640, 480)
        assert run() == capi.ERR_UNSUPPORTED and b"projection" in why()
        ctx.set_projection(None)
        for option, on, off, word in (("inlier_fraction", 0.5, 1.0, b"post-filters"), ("one_to_one", 1, 0, b"post-filters"), ("point_weight_evaluator", 2, 0, b"weights"),
                                      ("feature_normal_weight", 0.5, 0.0, b"feature adaptor")):
            ctx.set_option(option, on)
            assert run() == capi.ERR_UNSUPPORTED and word in why(), option
            ctx.set_option(option, off)
        assert (ctrl == 7).all()
        assert run() == capi.OK
    finally:
        ctx.close()


# ---- 8. the mirrors --------------------------------------------------------------------------------------------------------------------
def test_sparse_python_mirror_runs(case):
    from cilantro_amd.icp import SimpleCombinedMetricSparseAffineWarpFieldICP3f, transformPoints

    icp = SimpleCombinedMetricSparseAffineWarpFieldICP3f(case["dst"], case["dst_n"], case["src"], (case["ctrl_idx"], case["ctrl_d2"]), case["n_ctrl"], (case["reg_idx"], case["reg_d2"]))
    icp.correspondenceSearchEngine().setMaxDistance(case["max_sq"])
    icp.controlWeightEvaluator().setSigma(float(case["ctrl_sigma"]))
    icp.regularizationWeightEvaluator().setSigma(float(case["reg_sigma"]))
    icp.setMaxNumberOfIterations(3).setConvergenceTolerance(2.5e-3).setMaxNumberOfGaussNewtonIterations(1).setStiffnessRegularizationWeight(1.0).setHuberLossBoundary(1e-2)
    T = icp.estimate().getTransform()
    assert T.shape == (case["n_ctrl"], 4, 4) and np.isfinite(T).all() and 1 <= icp.getNumberOfPerformedIterations() <= 3
    assert np.abs(T[:, :3, :3] @ T[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() > 1e-5      # (affine: not polished)
    before = W.plane_residuals(case["dst"], case["dst_n"], case["src"]).mean()
    assert W.plane_residuals(case["dst"], case["dst_n"], transformPoints(icp.getDenseWarpField(), case["src"])).mean() < before
    res = icp.getResiduals()
    assert res.shape == (len(case["src"]),) and np.isfinite(res).all()


def test_dense_python_mirror_runs():
    from cilantro_amd import synthetic
    from cilantro_amd.icp import SimpleCombinedMetricDenseAffineWarpFieldICP3f, transformPoints

    src, _ = synthetic.make_surface(400, seed=45)
    flat, nrm = synthetic.make_surface(600, seed=46)
    dst = synthetic.bend(flat)
    icp = SimpleCombinedMetricDenseAffineWarpFieldICP3f(dst, nrm, src, W.knn_lists(src, src, 6))
    icp.correspondenceSearchEngine().setMaxDistance(0.1 ** 2)
    icp.regularizationWeightEvaluator().setSigma(0.2)
    icp.setMaxNumberOfIterations(3).setConvergenceTolerance(2.5e-3).setMaxNumberOfGaussNewtonIterations(1).setStiffnessRegularizationWeight(1.0).setHuberLossBoundary(1e-2)
    icp.setPointToPointMetricWeight(0.1)
    T = icp.estimate().getTransform()
    assert T.shape == (400, 4, 4) and np.isfinite(T).all() and 1 <= icp.getNumberOfPerformedIterations() <= 3
    before = W.plane_residuals(dst, nrm, src).mean()
    assert W.plane_residuals(dst, nrm, transformPoints(icp.getDenseWarpField(), src)).mean() < before


def test_resample_transforms_affine_switch(case):
    from cilantro_amd.icp import RBFKernelWeightEvaluator, resampleTransforms

    T = random_affine(case["n_ctrl"], 4)
    ev = RBFKernelWeightEvaluator()
    ev.setSigma(float(case["ctrl_sigma"]))
    got = resampleTransforms(T, (case["ctrl_idx"], case["ctrl_d2"]), ev, affine=True)
    assert np.abs(got - A.resample(case["graph"], T, F)).max() < 2e-6
    polished = resampleTransforms(T, (case["ctrl_idx"], case["ctrl_d2"]), ev)
    assert np.abs(polished[:, :3, :3] @ polished[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-5


def test_cpp_mirror_registers_a_bent_surface():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_warp_field_affine.cpp"), "test_warp_field_affine")
    r = subprocess.run([exe, "run"], capture_output=True, text=True)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
