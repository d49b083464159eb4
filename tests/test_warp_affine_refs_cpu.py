"""CPU: tests/_warp_affine_refs.py, the restatement the affine warp-field GPU tests compare against, pinned
down on its own: the vectorised assembly against the literal loops, the dense affine estimator's system as the k_ctrl = 1 special case,
sorted against list-order lists, the Jacobian against central differences -- exact at the identity, scaled by s_t / s per component
away from it (the reference's rows carry the transformed point) -- the matrix-free product, the no-data returns and the resample."""
import numpy as np
import pytest

import _warp_affine_refs as A
import _warp_refs as W

F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def case():
    c = W.make_case(n_src=400, n_dst=500, res=0.2)
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    rng = np.random.RandomState(7)
    c["tf"] = A.identity_start(c["n_ctrl"], D) + (rng.standard_normal((c["n_ctrl"], 12)) * np.array([0.02] * 9 + [0.004] * 3)).reshape(-1)
    return c


def prm(**kw):
    base = dict(w_p2p=0.1, w_p2pl=1.0, w_reg=1.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=1000, cg_conv_tol=1e-5)
    base.update(kw)
    return W.Params(**base)


def test_start_is_the_identity():
    tf = A.identity_start(3, F).reshape(3, 12)
    assert (tf[:, :9].reshape(3, 3, 3) == np.eye(3, dtype=F)).all() and not tf[:, 9:].any()
    assert (A.to_transforms(tf, F) == np.eye(4, dtype=F)).all()


@pytest.mark.parametrize("dtype, tol", [(D, 1e-13), (F, 2e-6)])
def test_vectorised_assembly_equals_the_literal_loops(case, dtype, tol):
    args = (case["graph"], dtype, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    At, b, info = A.assemble(*args)
    assert info["n_pt_eq"] == 3 * info["matches"] and info["n_pl_eq"] == info["matches"] and info["n_reg_eq"] == 12 * len(case["graph"].arc_s)
    M, bl = A.assemble_literal(*args)
    assert M.shape == At.T.shape
    assert np.abs(At.T.toarray() - M).max() <= tol * np.abs(M).max()
    assert np.abs(b - bl).max() <= tol * max(np.abs(bl).max(), 1e-30)


def test_dense_estimator_is_the_one_node_per_point_special_case():
    """50 points, every point its own control node (ctrl_idx[i] = i, k_ctrl = 1, Unity), k_reg = 6: the sparse affine system equals,
    term for term, the dense affine estimator's (:856-955)"""
    from cilantro_amd import synthetic

    src, _ = synthetic.make_surface(50, seed=45)
    flat, nrm = synthetic.make_surface(80, seed=46)
    dst = synthetic.bend(flat)
    reg_idx, reg_d2 = W.knn_lists(src, src, 6)
    sigma = F(0.3)
    g = W.Graph(50, np.arange(50, dtype=np.uint32)[:, None], np.zeros((50, 1), F), W.UNITY, 1.0, reg_idx, reg_d2, W.RBF, sigma)
    nn = W.nearest(dst, src, np.inf)
    tf = A.identity_start(50, D) + (np.random.RandomState(5).standard_normal((50, 12)) * 0.01).reshape(-1)
    for dtype, tol in ((D, 1e-14), (F, 1e-6)):
        At, b, _ = A.assemble(g, dtype, dst, nrm, src, nn, tf, prm())
        M, bd = A.assemble_dense_literal(dtype, dst, nrm, src, nn, reg_idx, np.sqrt(W.eval_weights(W.RBF, sigma, reg_d2)), tf, prm())
        assert M.shape == At.T.shape
        assert np.abs(At.T.toarray() - M).max() <= tol * np.abs(M).max()
        assert np.abs(b - bd).max() <= tol * np.abs(bd).max()


def test_sorted_lists_and_list_order_give_the_same_system(case):
    args = (case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    A1, b1, _ = A.assemble(*args, sort=True)
    A2, b2, _ = A.assemble(*args, sort=False)
    M1, M2 = (A1 @ A1.T).toarray(), (A2 @ A2.T).toarray()
    assert np.abs(M1 - M2).max() <= 1e-12 * np.abs(M1).max()
    assert np.abs(A1 @ b1 - A2 @ b2).max() <= 1e-12 * np.abs(A1 @ b1).max()


def _data_rows_central_differences(case, tf, p):
    """-(d b / d unknown) of the data rows for 72 unknowns drawn at random (every component class among them), f64 -> the rows' own
    columns, the quotients, info, the unknowns.  b is linear in the unknowns, so the step may be large and the quotient is exact up to
    rounding."""
    args = (case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"])
    At, b, info = A.assemble(*args, tf, p)
    nd = info["n_pt_eq"] + info["n_pl_eq"]
    cols = np.sort(np.random.RandomState(11).choice(At.shape[0], 72, replace=False))
    assert len(set(cols % 12)) == 12
    fd = np.zeros((nd, len(cols)))
    h = 1e-3
    for q, u in enumerate(cols):
        e = np.zeros(At.shape[0]); e[u] = h
        fd[:, q] = -(A.assemble(*args, tf + e, p)[1][:nd] - A.assemble(*args, tf - e, p)[1][:nd]) / (2 * h)
    return At.T.toarray()[:nd][:, cols], fd, info, cols


def test_at_the_identity_the_rows_are_the_true_jacobian(case):
    """tforms_vec = identity: s_t == s and the data rows equal the central differences of the residuals (the regularisation rows sit on
    the kink of |x| there, where a central difference says nothing; the literal transcription above covers them).
    "Equal" is to the rounding of the totals: total_i is DATA, the f32 sum of k_ctrl = 4 weights (three additions of half an ulp each,
    1.8e-7 relative), so the blend of identities is 1 to that and no closer, in any dtype."""
    J, fd, info, _ = _data_rows_central_differences(case, A.identity_start(case["n_ctrl"], D), prm())
    assert np.abs(info["s_t"] - info["s"]).max() <= 1.8e-7 * np.abs(info["s"]).max()
    assert np.abs(J).max() > 0.1 and np.abs(J - fd).max() <= 1.8e-7 * np.abs(J).max()


def test_away_from_the_identity_the_rows_are_the_jacobian_scaled_by_st_over_s(case):
    """the quirk as arithmetic: at a perturbed tforms_vec the coefficient at unknown 3 r + c of the linear part is the true derivative
    times s_t[c] / s[c] of the row's point; the translation's coefficients are the true derivatives"""
    J, fd, info, cols = _data_rows_central_differences(case, case["tf"], prm())
    s, s_t = info["s"], info["s_t"]
    m = len(s)
    point_of_row = np.concatenate([np.repeat(np.arange(m), 3), np.arange(m)])      # three point rows per match, then one plane row each
    assert len(point_of_row) == len(J)
    comp = cols % 12
    lin = comp < 9
    scale = np.ones_like(J)
    scale[:, lin] = (s_t / s)[point_of_row][:, comp[lin] % 3]
    assert np.abs(s_t / s - 1).max() > 1e-3      # (the case does tell the two apart)
    assert np.abs(J - fd * scale).max() <= 1e-10 * np.abs(J).max()
    assert np.abs(J - fd).max() > 1e-4 * np.abs(J).max()
    # and the variant built from s is the true Jacobian
    Js = A.assemble(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm(), jac_point="s")[0].T.toarray()[:len(J)][:, cols]
    assert np.abs(Js - fd).max() <= 1e-10 * np.abs(J).max()


def test_matrix_free_product_equals_the_explicit_one(case):
    At, b, info = A.assemble(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    AtA = (At @ At.T).toarray()
    p = np.random.RandomState(3).standard_normal(At.shape[0])
    want = AtA @ p
    assert np.abs(W.apply_matrix_free(At, p) - want).max() <= 1e-12 * np.abs(want).max()


def test_early_return_rules(case):
    g = case["graph"]
    none = np.full(len(case["src"]), W.NONE, np.uint32)
    for nn, p in ((none, prm()), (case["nn"], prm(w_p2p=0.0, w_p2pl=0.0))):
        tf, st = A.estimate(g, F, case["dst"], case["dst_n"], case["src"], nn, p)
        assert not st["data_term"] and not st["converged"] and st["gn_iterations"] == 0
        assert (A.to_transforms(tf, F) == np.eye(4, dtype=F)).all()


def test_estimate_reduces_the_plane_residual(case):
    p = prm(w_p2p=0.0, max_gn_iter=2)
    tf, st = A.estimate(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], p)
    warped = W.transform_points(A.resample(case["graph"], A.to_transforms(tf, D), D), case["src"])
    before, after = W.plane_residuals(case["dst"], case["dst_n"], case["src"]).mean(), W.plane_residuals(case["dst"], case["dst_n"], warped).mean()
    assert after < 0.9 * before, (before, after)


def test_resample_is_the_plain_blend(case):
    g = case["graph"]
    rng = np.random.RandomState(2)
    T = np.tile(np.eye(4), (case["n_ctrl"], 1, 1))
    T[:, :3, :] += rng.standard_normal((case["n_ctrl"], 3, 4)) * 0.1      # affine, far from a rotation
    dense = A.resample(g, T, D)
    # a literal blend of one point
    i = 17
    acc = sum(D(g.w[i, j]) * T[g.idx[i, j], :3, :] for j in range(g.idx.shape[1]) if g.valid[i, j]) * (1.0 / D(g.total[i]))
    assert np.abs(dense[i, :3] - acc).max() <= 1e-15 and (dense[:, 3] == [0, 0, 0, 1]).all()
    assert np.abs(dense[:, :3, :3] @ dense[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() > 1e-2      # (not polished)
    assert np.abs(A.resample(g, T, F) - dense).max() < 2e-6
    tiny = W.Graph(case["n_ctrl"], case["ctrl_idx"], case["ctrl_d2"], W.RBF, 1e-4, case["reg_idx"], case["reg_d2"], W.RBF, 1.0)
    dead = tiny.total == 0
    assert dead.any() and (A.resample(tiny, T, F)[dead] == np.eye(4, dtype=F)).all()
    assert np.abs(A.readback(A.to_transforms(case["tf"], D)).reshape(-1) - case["tf"]).max() == 0


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("dtype, tol", [(D, 1e-13), (F, 2e-6)])
def test_lattice_graph_vectorised_assembly_equals_the_literal_loops(dtype, tol, holes):
    """the graphs of tests/test_gpu_warp_field_edges.py (_warp_refs.make_lattice_case; tests/test_warp_refs_cpu.py pins its lists):
    ragged rows as they come, then with NONE in the middle of both kinds of list, a row without its owner and a matched source point
    that names no control node -- its rows are empty and its entries of b are 0 (:1924-1933, :2059-2071)"""
    c = W.make_lattice_case(7, 5, 3, 5, extra=45, seed=3)
    tf = A.identity_start(35, D) + (np.random.RandomState(8).standard_normal((35, 12)) * np.array([0.02] * 9 + [0.004] * 3)).reshape(-1)
    g = c["graph"]
    if holes:
        ci, ri = c["ctrl_idx"].copy(), c["reg_idx"].copy()
        ci[::3, 1] = W.NONE
        ci[2] = W.NONE
        ri[::4, 2] = W.NONE
        ri[9, 0] = W.NONE
        g = W.Graph(35, ci, c["ctrl_d2"], W.RBF, c["ctrl_sigma"], ri, c["reg_d2"], W.RBF, c["reg_sigma"])
        assert g.total[2] == 0 and c["nn"][2] != W.NONE
    args = (g, dtype, c["dst"], c["dst_n"], c["src"], c["nn"], tf, prm())
    At, b, info = A.assemble(*args)
    M, bl = A.assemble_literal(*args)
    assert info["matches"] == 80 - 7 and info["n_reg_eq"] == 12 * len(g.arc_s) and M.shape == At.T.shape
    assert np.abs(At.T.toarray() - M).max() <= tol * np.abs(M).max()
    assert np.abs(b - bl).max() <= tol * max(np.abs(bl).max(), 1e-30)
    if holes:
        pos = int((c["nn"][:2] != W.NONE).sum())
        rows = list(range(3 * pos, 3 * pos + 3)) + [info["n_pt_eq"] + pos]
        assert not M[rows].any() and not bl[rows].any()


def test_the_findings_the_gpu_cases_are_built_on():
    """On the GPU tests' pair (make_case(): 3 000 / 4 000 points, 286 nodes, 2 002 arcs), the restatements alone.
    The example's w_reg = 200 is unfit for affine solve tests: at max_cg_iter = 500, cg_conv_tol = 1e-5 the f32 restatement hits the cap
    (the f64 one stops at 492) and the two end 4.6e-3 apart -- no tolerance follows from that.  At w_reg = 1 with max_cg_iter = 1000 both
    stop on their own (cg_conv_tol = 1e-4: 396 and 373 iterations), apart in count: an iteration-count condition has to name both."""
    c = W.make_case()
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    assert (c["n_ctrl"], len(c["graph"].arc_s)) == (286, 2002)

    def run(dtype, **kw):
        return A.estimate(c["graph"], dtype, c["dst"], c["dst_n"], c["src"], c["nn"], prm(w_p2p=0.0, **kw))

    (t32, s32), (t64, s64) = run(F, w_reg=200.0, max_cg_iter=500), run(D, w_reg=200.0, max_cg_iter=500)
    assert s32["cg_iterations_total"] == 500 and 450 < s64["cg_iterations_total"] <= 500
    assert np.abs(t32.astype(D) - t64).max() > 1e-3
    (t32, s32), (t64, s64) = run(F, cg_conv_tol=1e-4), run(D, cg_conv_tol=1e-4)
    assert s64["cg_iterations_total"] < s32["cg_iterations_total"] < 1000
    assert s32["cg_iterations_total"] > 1.03 * s64["cg_iterations_total"]
    assert np.abs(t32.astype(D) - t64).max() < 1e-4
