"""CPU: tests/_warp_refs.py, the restatement the GPU warp-field tests compare against, pinned down on its own: the matrix-free product
against the explicit one, the Jacobian against finite differences of the residuals, sorted against list-order lists, the vectorised
assembly against the literal loops, the dense estimator's system as the k_ctrl = 1 special case, Eigen's CG against a direct solve, and
the early-return rules."""
import numpy as np
import pytest

import _warp_refs as W

F, D = np.float32, np.float64


@pytest.fixture(scope="module")
def case():
    c = W.make_case(n_src=400, n_dst=500, res=0.2)
    c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
    rng = np.random.RandomState(7)
    c["tf"] = (rng.standard_normal((c["n_ctrl"], 6)) * np.array([0.02, 0.02, 0.02, 0.004, 0.004, 0.004])).reshape(-1)
    return c


def prm(**kw):
    base = dict(w_p2p=0.1, w_p2pl=1.0, w_reg=200.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=500, cg_conv_tol=1e-5)
    base.update(kw)
    return W.Params(**base)


def test_case_shape(case):
    assert 10 <= case["n_ctrl"] <= 60 and (case["nn"] != W.NONE).sum() > 300
    assert (case["ctrl_idx"] != W.NONE).all() and (case["reg_idx"][:, 0] == np.arange(case["n_ctrl"])).all()      # self first


def test_matrix_free_product_equals_the_explicit_one(case):
    At, b, info = W.assemble(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    assert info["n_pt_eq"] == 3 * info["matches"] and info["n_pl_eq"] == info["matches"] and info["n_reg_eq"] == 6 * len(case["graph"].arc_s)
    AtA = (At @ At.T).toarray()
    p = np.random.RandomState(3).standard_normal(At.shape[0])
    want = AtA @ p
    assert np.abs(W.apply_matrix_free(At, p) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(AtA - AtA.T).max() == 0 or np.abs(AtA - AtA.T).max() <= 1e-12 * np.abs(AtA).max()


@pytest.mark.parametrize("hb", [1e-2, 1e-3])
def test_jacobian_rows_against_finite_differences(case, hb):
    """b = -residual and At^T = d residual / d unknown: central differences of b in f64.  (Unknowns exactly at a Huber kink do not occur:
    the perturbed tforms_vec is random.)"""
    g, p = case["graph"], prm(huber_boundary=hb)
    args = (g, D, case["dst"], case["dst_n"], case["src"], case["nn"])
    At, b, info = W.assemble(*args, case["tf"], p)
    assert all(info["huber_branches"]) or hb == 1e-2
    J = At.T.toarray()
    h = 1e-6
    rng = np.random.RandomState(11)
    for u in rng.choice(At.shape[0], 12, replace=False):
        e = np.zeros(At.shape[0]); e[u] = h
        bp, bm = W.assemble(*args, case["tf"] + e, p)[1], W.assemble(*args, case["tf"] - e, p)[1]
        fd = -(bp - bm) / (2 * h)
        assert np.abs(fd - J[:, u]).max() <= 2e-6 * max(1.0, np.abs(J[:, u]).max()), u


def test_sorted_lists_and_list_order_give_the_same_system(case):
    args = (case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    A1, b1, _ = W.assemble(*args, sort=True)
    A2, b2, _ = W.assemble(*args, sort=False)
    M1, M2 = (A1 @ A1.T).toarray(), (A2 @ A2.T).toarray()
    assert np.abs(M1 - M2).max() <= 1e-12 * np.abs(M1).max()
    assert np.abs(A1 @ b1 - A2 @ b2).max() <= 1e-12 * np.abs(A1 @ b1).max()


@pytest.mark.parametrize("dtype, tol", [(D, 1e-13), (F, 2e-6)])
def test_vectorised_assembly_equals_the_literal_loops(case, dtype, tol):
    args = (case["graph"], dtype, case["dst"], case["dst_n"], case["src"], case["nn"], case["tf"], prm())
    At, b, _ = W.assemble(*args)
    A, bl = W.assemble_literal(*args)
    assert A.shape == At.T.shape
    assert np.abs(At.T.toarray() - A).max() <= tol * np.abs(A).max()
    assert np.abs(b - bl).max() <= tol * max(np.abs(bl).max(), 1e-30)


def test_dense_estimator_is_the_one_node_per_point_special_case():
    """50 points, every point its own control node (ctrl_idx[i] = i, k_ctrl = 1, Unity), k_reg = 6: the sparse system equals, term for
    term, the dense estimator's (:369-716)"""
    from cilantro_amd import synthetic

    src, _ = synthetic.make_surface(50, seed=45)
    flat, nrm = synthetic.make_surface(80, seed=46)
    dst = synthetic.bend(flat)
    reg_idx, reg_d2 = W.knn_lists(src, src, 6)
    sigma = F(0.3)
    g = W.Graph(50, np.arange(50, dtype=np.uint32)[:, None], np.zeros((50, 1), F), W.UNITY, 1.0, reg_idx, reg_d2, W.RBF, sigma)
    nn = W.nearest(dst, src, np.inf)
    tf = (np.random.RandomState(5).standard_normal((50, 6)) * 0.01).reshape(-1)
    for dtype, tol in ((D, 1e-14), (F, 1e-6)):
        At, b, _ = W.assemble(g, dtype, dst, nrm, src, nn, tf, prm())
        A, bd = W.assemble_dense_literal(dtype, dst, nrm, src, nn, reg_idx, np.sqrt(W.eval_weights(W.RBF, sigma, reg_d2)), tf, prm())
        assert A.shape == At.T.shape
        assert np.abs(At.T.toarray() - A).max() <= tol * np.abs(A).max()
        assert np.abs(b - bd).max() <= tol * np.abs(bd).max()


def test_eigen_cg_meets_its_promise_and_matches_a_direct_solve(case):
    At, b, _ = W.assemble(case["graph"], D, case["dst"], case["dst_n"], case["src"], case["nn"], np.zeros(6 * case["n_ctrl"]), prm(w_p2p=0.0))
    AtA, Atb = (At @ At.T).tocsc(), At @ b
    x, its, res2 = W.eigen_cg(AtA, Atb, 1e-10, 2000, D)
    assert 0 < its < 2000
    assert np.linalg.norm(AtA @ x - Atb) <= 2e-10 * np.linalg.norm(Atb)
    direct = np.linalg.solve(AtA.toarray(), Atb)
    assert np.abs(x - direct).max() <= 1e-6 * np.abs(direct).max()
    # one iteration: x1 = alpha M^-1 A^T b
    x1, its1, _ = W.eigen_cg(AtA, Atb, 1e-10, 1, D)
    z = Atb / AtA.diagonal()
    assert its1 == 1 and np.allclose(x1, (Atb @ z) / (z @ (AtA @ z)) * z, rtol=1e-12, atol=0)
    # a zero right-hand side, and a zero diagonal entry (M^-1 = 1 there)
    assert W.eigen_cg(AtA, np.zeros(len(Atb)), 1e-5, 10, D)[1] == 0
    Z = AtA.tolil(); Z[0, :] = 0; Z[:, 0] = 0
    rhs = Atb.copy(); rhs[0] = 0
    assert W.eigen_cg(Z.tocsc(), rhs, 1e-8, 2000, D)[0][0] == 0


def test_early_return_rules(case):
    g = case["graph"]
    none = np.full(len(case["src"]), W.NONE, np.uint32)
    for nn, p in ((none, prm()), (case["nn"], prm(w_p2p=0.0, w_p2pl=0.0))):
        tf, st = W.estimate(g, F, case["dst"], case["dst_n"], case["src"], nn, p)
        assert not st["data_term"] and not st["converged"] and st["gn_iterations"] == 0 and not tf.any()
        T = W.to_transforms(tf, F)
        assert (T == np.eye(4, dtype=F)).all()


def test_estimate_reduces_the_plane_residual_and_f32_follows_f64(case):
    p = prm(w_p2p=0.0, max_gn_iter=3)
    out = {}
    for dtype in (F, D):
        tf, st = W.estimate(case["graph"], dtype, case["dst"], case["dst_n"], case["src"], case["nn"], p)
        out[dtype] = tf
        dense = W.resample(case["graph"], W.to_transforms(tf, dtype), dtype)
        warped = W.transform_points(dense, case["src"])
        before, after = W.plane_residuals(case["dst"], case["dst_n"], case["src"]).mean(), W.plane_residuals(case["dst"], case["dst_n"], warped).mean()
        assert after < 0.9 * before, (before, after)      # (a coarse, stiff field on a sparsely sampled surface: the sampling floor stays)
    assert np.abs(out[F] - out[D]).max() <= 1e-3 * np.abs(out[D]).max()


def test_utilities(case):
    g = case["graph"]
    tf = case["tf"]
    T = W.to_transforms(tf, D)
    assert np.abs(T[:, :3, :3] @ T[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    assert np.abs(W.angles_of(T) - tf.reshape(-1, 6)[:, :3]).max() < 1e-12 and (T[:, :3, 3] == tf.reshape(-1, 6)[:, 3:]).all()
    dense = W.resample(g, T, D)
    assert np.abs(dense[:, :3, :3] @ dense[:, :3, :3].transpose(0, 2, 1) - np.eye(3)).max() < 1e-13
    tiny = W.Graph(case["n_ctrl"], case["ctrl_idx"], case["ctrl_d2"], W.RBF, 1e-4, case["reg_idx"], case["reg_d2"], W.RBF, 1.0)
    dead = tiny.total == 0
    assert dead.any() and (W.resample(tiny, T, F)[dead] == np.eye(4, dtype=F)).all()
    I = np.tile(np.eye(4, dtype=F), (len(case["src"]), 1, 1))
    assert (W.transform_points(I, case["src"]) == case["src"]).all()
    T2, d2 = W.compose(T, T, D)
    assert np.allclose(T2, T @ T) and d2 > 0
