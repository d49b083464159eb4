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


# ---- the lattice builder of tests/test_gpu_warp_field_edges.py -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lattice():
    c = W.make_lattice_case(7, 5, 3, 5, extra=45, seed=3)
    c["tf"] = (np.random.RandomState(8).standard_normal((c["n_ctrl"], 6)) * np.array([0.02, 0.02, 0.02, 0.004, 0.004, 0.004])).reshape(-1)
    return c


def test_lattice_case_shape(lattice):
    c = lattice
    assert c["n_ctrl"] == 35 and len(c["src"]) == len(c["dst"]) == len(c["dst_n"]) == 80 and c["ctrl_idx"].shape == (80, 3) and c["reg_idx"].shape == (35, 5)
    assert np.abs(np.linalg.norm(c["dst_n"], axis=1) - 1).max() < 1e-6
    assert (c["nn"][5::11] == W.NONE).all() and (np.delete(c["nn"], np.arange(5, 80, 11)) == np.delete(np.arange(80), np.arange(5, 80, 11))).all()
    assert W.lattice_offsets(4) == [(0, -1), (-1, 0), (1, 0), (0, 1)] and len(set(W.lattice_offsets(31))) == 31
    assert max(dx * dx + dy * dy for dx, dy in W.lattice_offsets(31)) == 10      # (none nearer is left out: 36 steps have a norm^2 <= 10, 28 one <= 9)
    # the matches are real ones: the target point stands within the case's search radius of its source point
    m = c["nn"] != W.NONE
    assert (W.d2_pairs(c["src"][m], c["dst"][c["nn"][m]]) < c["max_sq"]).all()


@pytest.mark.parametrize("k", [1, 3, 32])
def test_lattice_control_lists_equal_knn_lists(k):
    """wherever the listed distances and the first one left out are distinct, in the pinned f32 expression"""
    c = W.make_lattice_case(20, 15, k, 2, extra=300, seed=31)
    idx, d2 = W.knn_lists(c["ctrl"], c["src"], k)
    full = np.sort(W.d2_pinned(c["src"], c["ctrl"]), axis=1)[:, :k + 1]
    distinct = (np.diff(full, axis=1) > 0).all(1)
    assert distinct.mean() > 0.9
    assert (c["ctrl_idx"][distinct] == idx[distinct]).all() and (c["ctrl_d2"][distinct] == d2[distinct]).all()
    assert (np.sort(c["ctrl_idx"], axis=1) == np.sort(idx, axis=1)).mean() > 0.99      # (a tie may swap two equal distances, no more)
    small = W.make_lattice_case(2, 1, 4, 5, extra=3, seed=1)      # lists wider than the lattice: padded
    assert (small["ctrl_idx"][:, 2:] == W.NONE).all() and (np.sort(small["ctrl_idx"][:, :2], axis=1) == [0, 1]).all() and (small["ctrl_d2"][:, 2:] == 0).all()


def test_lattice_regularisation_rows(lattice):
    """row i = [i, lattice neighbours..., NONE...], ragged at the border; the listed d2 are the pinned ones; where the four lattice
    neighbours are nearer than every other node (the surface is curved) the row is knn_lists' row as a set"""
    c = lattice
    ri, rd = c["reg_idx"], c["reg_d2"]
    Dm = W.d2_pinned(c["ctrl"], c["ctrl"])
    assert (ri[:, 0] == np.arange(35)).all() and (rd[:, 0] == 0).all()
    count = (ri != W.NONE).sum(1)
    assert sorted(set(count)) == [3, 4, 5] and (count == 3).sum() == 4 and (count == 5).sum() == 5 * 3      # corners, edges, interior
    knn = W.knn_lists(c["ctrl"], c["ctrl"], 5)[0]
    same = 0
    for i in range(35):
        row = ri[i, :count[i]].astype(np.int64)
        assert (ri[i, count[i]:] == W.NONE).all() and (rd[i, count[i]:] == 0).all()      # padding last
        assert all(abs(j % 7 - i % 7) + abs(j // 7 - i // 7) == 1 for j in row[1:])
        assert (rd[i, :count[i]] == Dm[i, row]).all()
        others = np.setdiff1d(np.arange(35), row)
        if count[i] == 5 and Dm[i, row].max() < Dm[i, others].min():
            same += 1
            assert set(row) == set(knn[i].astype(np.int64))
    assert same >= 8
    g = c["graph"]
    assert len(g.arc_s) == (count - 1).sum() == 2 * (6 * 5 + 7 * 4)      # every lattice edge twice: once from either end


@pytest.mark.parametrize("dtype, tol", [(D, 1e-13), (F, 2e-6)])
def test_lattice_graph_vectorised_assembly_equals_the_literal_loops(lattice, dtype, tol):
    c = lattice
    args = (c["graph"], dtype, c["dst"], c["dst_n"], c["src"], c["nn"], c["tf"], prm())
    At, b, info = W.assemble(*args)
    A, bl = W.assemble_literal(*args)
    assert info["matches"] == 80 - 7 and A.shape == At.T.shape
    assert np.abs(At.T.toarray() - A).max() <= tol * np.abs(A).max()
    assert np.abs(b - bl).max() <= tol * max(np.abs(bl).max(), 1e-30)


def test_lists_with_holes_and_empty_lists_assemble_as_the_literal_loops(lattice):
    """NONE in the middle of both kinds of list, a row without its owner, a matched source point with no control node at all: the
    literal loops skip what is not there, the point's rows are empty and its entries of b are 0 (:1456-1465, :1593-1596, :1687-1690)"""
    c = lattice
    ci, ri = c["ctrl_idx"].copy(), c["reg_idx"].copy()
    ci[::3, 1] = W.NONE
    ci[2] = W.NONE
    ri[::4, 2] = W.NONE
    ri[9, 0] = W.NONE
    g = W.Graph(35, ci, c["ctrl_d2"], W.RBF, c["ctrl_sigma"], ri, c["reg_d2"], W.RBF, c["reg_sigma"])
    assert g.total[2] == 0 and c["nn"][2] != W.NONE and (9, 10) not in g.directed and (10, 9) in g.directed
    args = (g, D, c["dst"], c["dst_n"], c["src"], c["nn"], c["tf"], prm())
    At, b, info = W.assemble(*args)
    A, bl = W.assemble_literal(*args)
    assert np.abs(At.T.toarray() - A).max() <= 1e-13 * np.abs(A).max() and np.abs(b - bl).max() <= 1e-13 * np.abs(bl).max()
    pos = int((c["nn"][:2] != W.NONE).sum())      # point 2's place among the matches
    rows = list(range(3 * pos, 3 * pos + 3)) + [info["n_pt_eq"] + pos]
    assert not A[rows].any() and not b[rows].any()


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
