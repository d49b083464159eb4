"""GPU: the spectral-clustering entries (cilhip_nn_graph_matrix, cilhip_sparse_*, cilhip_spectral_embedding, cilhip_kmeans_nd and their
Python / C++ mirrors) against tests/_spectral_refs.py -- DESIGN.md section 18, rules S1-S6 of c_api.h.  The neighbour lists come from
cilhip_knn3f (the builder is checked GIVEN the lists); eigenpairs are compared with dense f64 numpy.linalg.eigh of the same f32-valued matrix.
Every bound is derived where it is used; each test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _spectral_refs as R
from cilantro_amd import capi
from test_components_refs_cpu import build_cpp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
SMALL = ["blobs3", "blobs5", "shells", "uniform"]
TYPES = [R.UNNORMALIZED, R.NORMALIZED_SYMMETRIC, R.NORMALIZED_RANDOM_WALK]
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def lists(name):
    """(idx uint32 [n, k] padded with 0xFFFFFFFF, d2 f32 [n, k]) of cilhip_knn3f"""
    def make():
        from cilantro_amd.normal_estimation import KDTree3f

        P, _ = R.cloud(name)
        idx, d2, _ = KDTree3f(P).kNNSearch(None, R.INPUTS[name][1])
        return (idx & 0xFFFFFFFF).astype(np.uint32), d2
    return cached(("lists", name), make)


def affinities(name):
    """the symmetric RBF (sigma 1) graph of an input, built on the device (kept for the whole module)"""
    from cilantro_amd import clustering as cl

    return cached(("W", name), lambda: cl.nn_graph_sparse_matrix(lists(name), cl.RBFKernelWeightEvaluator(1.0), True))


def spectrum(name, kind):
    """dense f64: (eigenvalues, eigenvectors, upper bound, degrees) of the operator the device solves (the random-walk type: its symmetric form)"""
    def make():
        off, col, val = affinities(name).get()
        A, ub, d = R.laplacian(R.dense(len(off) - 1, off, col, val), kind)
        lam, Q = np.linalg.eigh(A)
        return lam, Q, ub, d, A
    return cached(("eigh", name, min(kind, 1)), make)


def embed(name, kind, max_clusters, estimate):
    from cilantro_amd import clustering as cl

    return cached(("embed", name, kind, max_clusters, estimate), lambda: cl.spectral_embedding(affinities(name), max_clusters, estimate, kind))


# ---- 1: S1 -----------------------------------------------------------------------------------------------------------------------------
def _graph_case(name, layout, on_device, kind, sym, duplicates):
    from cilantro_amd import clustering as cl

    idx, d2 = lists(name)
    n = len(idx)
    ev = [cl.UnityWeightEvaluator(), cl.IdentityWeightEvaluator(), cl.RBFKernelWeightEvaluator(1.0)][kind]
    if layout == "csr":
        off, ci, cd = R.lists_to_csr(idx, d2)
        want = R.graph_csr(n, ci, cd, off, kind, 1.0, sym, duplicates)
        arg = (off, ci, cd)
    else:
        want = R.graph_csr(n, idx, d2, None, kind, 1.0, sym, duplicates)
        arg = (idx, d2)
    if on_device:
        import torch

        arg = tuple(torch.from_numpy(a.astype(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for a in arg)
    M = cl.nn_graph_sparse_matrix(arg, ev, sym, duplicates)
    got = M.get(on_device)
    if on_device:
        got = (got[0].cpu().numpy().astype(np.uint64), got[1].cpu().numpy().view(np.uint32), got[2].cpu().numpy())
    info = M.info()
    M.close()
    assert info == (n, len(want[1]), int(np.diff(want[0].astype(np.int64)).max()))
    for g, w, what in zip(got, want, ("offsets", "columns", "values")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (name, layout, on_device, kind, sym, duplicates, what)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout", ["knn", "csr"])
@pytest.mark.parametrize("name", ["blobs3", "uniform"])
def test_graph_matrix_bit_for_bit(name, layout, on_device):
    """S1: offsets, columns and values of the device build equal the restatement's byte for byte -- both list layouts, Unity / Identity /
    RBF, with and without forced symmetry, both duplicates rules, host and device arrays"""
    for kind in (R.UNITY, R.IDENTITY, R.RBF):
        for sym in (False, True):
            for duplicates in (0, 1):
                _graph_case(name, layout, on_device, kind, sym, duplicates)


def test_graph_matrix_with_lists_that_repeat_and_pad():
    """a list that names a point twice (three values meet on one entry: summed in list order, or the last one assigned) and a short list"""
    from cilantro_amd import clustering as cl

    idx, d2 = (a.copy() for a in lists("blobs3"))
    idx[5, 6:] = R.NONE
    idx[7, 3] = idx[7, 2]
    for duplicates in (0, 1):
        want = R.graph_csr(len(idx), idx, d2, None, R.RBF, 0.7, True, duplicates)
        M = cl.nn_graph_sparse_matrix((idx, d2), cl.RBFKernelWeightEvaluator(0.7), True, duplicates)
        got = M.get()
        M.close()
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_graph_matrix_past_one_grid_trip():
    """blocks7: 70 000 rows, more than one trip of every builder kernel's grid"""
    idx, d2 = lists("blocks7")
    want = R.graph_csr(len(idx), idx, d2, None, R.RBF, 1.0, True, 0)
    got = affinities("blocks7").get()
    assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def test_graph_refusals_found_on_the_device():
    from cilantro_amd import clustering as cl

    idx, d2 = (a.copy() for a in lists("blobs3"))
    idx[17, 2] = len(idx)
    with pytest.raises(capi.CilhipError, match="not below n"):
        cl.nn_graph_sparse_matrix((idx, d2), None, True)
    off, ci, cd = R.lists_to_csr(*lists("blobs3"))
    off = off.copy()
    off[5], off[6] = off[6], off[5]
    with pytest.raises(capi.CilhipError, match="offsets"):
        cl.nn_graph_sparse_matrix((off, ci, cd), None, True)


def test_from_csr_round_trip_and_device_rules():
    import torch
    from cilantro_amd import clustering as cl

    off, col, val = affinities("blobs3").get()
    for on_device in (False, True):
        args = (torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(col.view(np.int32)).cuda(), torch.from_numpy(val).cuda()) if on_device else (off, col, val)
        M = cl.SparseMatrix.from_csr(len(off) - 1, *args)
        got = M.get()
        assert M.info() == affinities("blobs3").info() and all(g.tobytes() == w.tobytes() for g, w in zip(got, (off, col, val)))
        M.close()
    bad = col.copy()
    bad[1], bad[2] = bad[2], bad[1]      # (the rules of a DEVICE matrix are checked on the device)
    with pytest.raises(capi.CilhipError, match="ascending"):
        cl.SparseMatrix.from_csr(len(off) - 1, torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(bad.view(np.int32)).cuda(), torch.from_numpy(val).cuda())


# ---- 2: eigenvalues ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", TYPES, ids=["unnormalized", "symmetric", "random_walk"])
@pytest.mark.parametrize("name", SMALL)
def test_eigenvalues(name, kind):
    """|lambda_out,i - max(lambda_ref,i, 0)| <= 1e-7 max(FLT_EPSILON^(2/3), lambda_ref,i) + 2^-24 lambda_ref,i + 1e-11 ub: a symmetric Ritz
    value lies within its residual of an eigenvalue (S4's criterion), the rounding to f32, the f64 roundoff of an operator of norm <= ub.
    A missed copy of a repeated zero eigenvalue fails this by the spectral gap (5 to 6 orders of magnitude above the bound).
    Measured on an MI355X (first run): error / bound at most 0.36 (shells, symmetric, third value), 0 on every zero eigenvalue; 6 to 9 outer
    iterations, 126 to 201 block products."""
    nev = R.INPUTS[name][2]
    lam, _, ub, _, _ = spectrum(name, kind)
    _, ev, info = embed(name, kind, nev, False)
    err = np.abs(ev.astype(F64) - np.maximum(lam[:nev], 0.0))
    bound = R.eigenvalue_bound(lam[:nev], ub)
    print(name, kind, "outer", info["outer_iterations"], "products", info["block_products"], "max residual %.3g" % info["max_residual"], "err / bound", np.round(err / bound, 4))
    assert ev.dtype == F32 and len(ev) == nev and info["n_converged"] == nev and info["num_eigenvalues"] == nev and info["num_clusters"] == nev
    assert (ev >= 0).all() and (np.diff(ev) >= 0).all()
    assert (err <= bound).all(), (err, bound)


# ---- 3: vectors ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [R.UNNORMALIZED, R.NORMALIZED_RANDOM_WALK], ids=["unnormalized", "random_walk"])
@pytest.mark.parametrize("name", SMALL)
def test_vectors(name, kind):
    """the returned pairs (the random-walk vectors scaled back by sqrt(d)) against the f64 operator:
    residual  ||A x_i - lambda_out,i x_i|| <= crit_i + 2^-23 ub ||x_i||   (S4's criterion; lambda and x each rounded to f32: 2^-25 ub + 2^-24 ub)
    orthonormality to 1e-6
    distance of x_i from the f64 eigenspace of the wanted set <= (sum_i bound_i^2)^1/2 / delta + 2^-23   (Davis-Kahan, delta = the gap behind
    the wanted set in the f64 spectrum; the f32 rounding of a unit vector)
    Measured on an MI355X (first run): residual / bound at most 0.104, orthonormality 1.4e-8 to 9.7e-8, distance / bound at most 0.0012
    (delta from 0.0039, blobs5 random walk, to 1.22, shells unnormalised)."""
    nev = R.INPUTS[name][2]
    lam, Q, ub, d, A = spectrum(name, kind)
    E, ev, info = embed(name, kind, nev, False)
    X = E.astype(F64) * (np.sqrt(d)[:, None] if kind == R.NORMALIZED_RANDOM_WALK else 1.0)
    norms = np.linalg.norm(X, axis=0)
    res = np.linalg.norm(A @ X - X * ev.astype(F64)[None, :], axis=0)
    bound = R.criterion(ev) + 2.0 ** -23 * ub * norms
    orth = np.abs(X.T @ X - np.eye(nev)).max()
    delta = lam[nev] - lam[nev - 1]
    dist = np.linalg.norm(X - Q[:, :nev] @ (Q[:, :nev].T @ X), axis=0)
    dist_bound = np.sqrt((bound ** 2).sum()) / delta + 2.0 ** -23
    print(name, kind, "residual / bound", np.round(res / bound, 4), "orth %.3g" % orth, "delta %.4g" % delta, "distance / bound", np.round(dist / dist_bound, 5))
    assert E.shape == (len(d), nev) and E.dtype == F32
    assert (res <= bound).all(), (res, bound)
    assert orth <= 1e-6
    assert (dist <= dist_bound).all(), (dist, dist_bound)
    big = np.abs(X).argmax(0)      # S5's sign rule, where the largest component is not a near tie
    assert all(X[big[c], c] > 0 for c in range(nev) if np.sort(np.abs(X[:, c]))[-2] < 0.999 * np.abs(X[big[c], c]))


# ---- 4: the symmetric type ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_symmetric_rows_have_unit_norm(name):
    nev = R.INPUTS[name][2]
    for args in ((nev, False), (nev - 1, True)):
        E, _, _ = embed(name, R.NORMALIZED_SYMMETRIC, *args)
        norms = np.linalg.norm(E.astype(F64), axis=1)
        print(name, args, "row norms in [%.9f, %.9f]" % (norms.min(), norms.max()))
        assert np.abs(norms - 1.0).max() <= 1e-6


@pytest.mark.parametrize("name", ["blobs3", "blobs5"])
def test_symmetric_embedding_is_the_component_indicator(name):
    """with as many vectors as components the normalised rows of one component coincide and those of two components are orthogonal:
    |E E^T - [same component]| <= 8 (||R||_F / delta) / min_row_norm + 2^-21.  ||R||_F <= (k crit(0)^2)^1/2 (S4 accepted every pair), delta =
    the first non-zero eigenvalue (Davis-Kahan for the null space), min_row_norm = the shortest row of the exact null-space basis
    D^1/2 1_c / ||.||: an error eps in a row of length r moves the normalised row by <= 2 eps / r, a product of two rows by twice that,
    sqrt(2) for sin Theta -> vectors; 2^-21 for the f32 rounding and normalisation.
    Measured on an MI355X (first run): 3.2e-7 against 4.84e-7 (blobs3), 2.84e-7 against 4.88e-7 (blobs5); row norms within 1.6e-7 of 1."""
    k = len(np.unique(R.cloud(name)[1]))
    planted = R.cloud(name)[1]
    lam, _, _, d, _ = spectrum(name, R.NORMALIZED_SYMMETRIC)
    E, ev, info = embed(name, R.NORMALIZED_SYMMETRIC, R.INPUTS[name][2] - 1, True)
    assert info["num_clusters"] == k and E.shape[1] == k
    vol = np.bincount(planted, weights=d)
    min_row = np.sqrt(d / vol[planted]).min()
    r_f = np.sqrt(k) * float(R.criterion(0.0))
    bound = 8.0 * (r_f / lam[k]) / min_row + 2.0 ** -21
    G = E.astype(F64) @ E.astype(F64).T
    err = np.abs(G - (planted[:, None] == planted[None, :])).max()
    print(name, "|E E^T - indicator| %.3g" % err, "bound %.3g" % bound, "delta %.4g" % lam[k], "min row norm %.4g" % min_row)
    assert err <= bound


# ---- 5: end to end -------------------------------------------------------------------------------------------------------------------------
def _first_of_each(planted):
    return [int(np.flatnonzero(planted == c)[0]) for c in np.unique(planted)]


@pytest.mark.parametrize("name,max_clusters", [("blobs3", 4), ("blobs5", 5), ("shells", 4)])
def test_end_to_end_finds_the_planted_partition(name, max_clusters):
    """estimation on, random-walk type, k-means started at the lowest point of each planted part: the number of clusters and every label"""
    from cilantro_amd import clustering as cl

    planted = R.cloud(name)[1]
    sc = cl.SpectralClustering(affinities(name), max_clusters, True, cl.GraphLaplacianType.NORMALIZED_RANDOM_WALK, initial_centroid_indices=_first_of_each(planted))
    k = len(np.unique(planted))
    print(name, "clusters", sc.getNumberOfClusters(), "eigenvalues", sc.getComputedEigenValues(), "k-means iterations", sc.getNumberOfPerformedIterations(), sc.embedding_info_)
    assert sc.getNumberOfClusters() == k and sc.getEmbeddingDimension() == k and sc.getEmbeddedPoints().shape == (len(planted), k)
    assert len(sc.getComputedEigenValues()) == max_clusters + 1
    assert (sc.getPointToClusterIndexMap() == planted).all()
    assert [len(c) for c in sc.getClusterToPointIndicesMap()] == np.bincount(planted).tolist()
    _cache[("sc", name)] = sc


def blocks7_clustering():
    from cilantro_amd import clustering as cl

    planted = R.cloud("blocks7")[1]
    return cached(("sc", "blocks7"), lambda: cl.SpectralClustering(affinities("blocks7"), 7, False, cl.GraphLaplacianType.NORMALIZED_RANDOM_WALK,
                                                                  initial_centroid_indices=_first_of_each(planted)))


def test_end_to_end_seven_blocks_of_ten_thousand():
    """max 7 without estimation: 7 clusters of 10 000, every pair converged.  Measured on an MI355X (first run): 28 outer iterations, 676
    block products, largest residual 1.9e-12, 30.7 ms for the embedding."""
    sc = blocks7_clustering()
    print("blocks7", sc.embedding_info_, sc.getComputedEigenValues())
    assert sc.embedding_info_["n_converged"] == 7 and sc.embedding_info_["num_eigenvalues"] == 7
    assert sc.getNumberOfClusters() == 7 and [len(c) for c in sc.getClusterToPointIndicesMap()] == [10000] * 7
    assert (sc.getPointToClusterIndexMap() == R.cloud("blocks7")[1]).all()
    assert (sc.getComputedEigenValues() <= float(R.eigenvalue_bound(0.0, 2.0))).all()      # seven components: seven zero eigenvalues


def test_dense_and_csr_inputs_of_the_mirror():
    from cilantro_amd import clustering as cl

    off, col, val = affinities("blobs3").get()
    planted = R.cloud("blobs3")[1]
    a = cl.SpectralClustering((off, col, val), 4, True, initial_centroid_indices=[0, 100, 200])
    b = cl.SpectralClustering(R.dense(300, off, col, val).astype(F32), 4, True, initial_centroid_indices=[0, 100, 200], kmeans_use_kd_tree=True)
    assert (a.getPointToClusterIndexMap() == planted).all() and (b.getPointToClusterIndexMap() == planted).all()
    assert a.getEmbeddedPoints().tobytes() == b.getEmbeddedPoints().tobytes()
    c = cl.SpectralClustering(affinities("blobs3"), 3, seed=5)      # the reference's random start: some partition into 3 non-empty parts
    assert c.getNumberOfClusters() == 3 and len(np.unique(c.getPointToClusterIndexMap())) <= 3


def test_cpp_mirror_clusters_three_blobs():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_spectral.cpp"), "test_spectral")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "run OK: 3 clusters" in r.stdout, r.stdout + r.stderr


# ---- 6: k-means in D dimensions ----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    return np.abs(a.astype(F64) - b.astype(F64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(F32)).astype(F64)


def _kmeans_case(x, start, max_iter=100, tol=R.FLT_EPS):
    from cilantro_amd import clustering as cl

    want_c, want_l, want_it = R.kmeans_nd(x, start, max_iter, tol)
    km = cl.KMeansXf(x).cluster(start, max_iter, tol)
    ok = np.isfinite(want_c)
    print("k-means", x.shape, "iterations", km.getNumberOfPerformedIterations(), want_it, "labels differing", int((km.getPointToClusterIndexMap() != want_l).sum()),
          "centroid ulps", _ulps(km.getClusterCentroids()[ok], want_c[ok]).max())
    assert (km.getPointToClusterIndexMap() == want_l).all() and km.getNumberOfPerformedIterations() == want_it
    assert (np.isfinite(km.getClusterCentroids()) == ok).all() and (km.getClusterCentroids().view(np.uint32)[ok] == want_c.view(np.uint32)[ok]).all()
    return km


def test_kmeans_nd_on_a_five_dimensional_embedding():
    """335 x 5 (blobs5's embedding): label for label against the restatement, finite centroids bit for bit; a start that empties a cluster.
    Measured on an MI355X (first run, here and at 70 000 x 7): no label differs, centroids 0 ulp apart, equal iteration counts."""
    E, _, info = embed("blobs5", R.NORMALIZED_RANDOM_WALK, 5, True)
    assert E.shape == (335, 5)
    km = _kmeans_case(E, E[_first_of_each(R.cloud("blobs5")[1])])
    assert (km.getPointToClusterIndexMap() == R.cloud("blobs5")[1]).all()
    start = E[[0, 1, 2, 70, 140]].copy()
    start[4] = 10.0      # nobody's nearest centroid: cluster 4 is empty after the first pass and gets repaired
    _kmeans_case(E, start)
    _kmeans_case(E, start, max_iter=1, tol=0.0)
    x = np.random.default_rng(2).standard_normal((335, 5)).astype(F32)      # points that are not in five tight clumps
    _kmeans_case(x, x[:6].copy(), max_iter=7)


def test_kmeans_nd_on_seventy_thousand_points_in_seven_dimensions():
    """70 000 x 7 (blocks7's embedding): more than one trip of the assignment's grid, every chunk of the sums"""
    E = blocks7_clustering().getEmbeddedPoints()
    assert E.shape == (70000, 7)
    _kmeans_case(E, E[_first_of_each(R.cloud("blocks7")[1])])
    start = E[[0, 5, 10000, 20000, 30000, 40000, 50000]].copy()
    start[1] = -3.0      # empty after the first pass
    _kmeans_case(E, start, max_iter=4)


def test_kmeans_xf_in_three_dimensions_agrees_with_kmeans3f():
    from cilantro_amd import clustering as cl

    P, planted = R.cloud("blobs3")
    start = P[[0, 1, 250]].copy()
    a = cl.KMeansXf(P).cluster(start.copy())
    b = cl.KMeans3f(P).cluster(start.copy())
    assert (a.getPointToClusterIndexMap() == b.getPointToClusterIndexMap()).all() and a.getNumberOfPerformedIterations() == b.getNumberOfPerformedIterations()
    assert (_ulps(a.getClusterCentroids(), b.getClusterCentroids()) <= 1.0).all()
    import torch

    c = cl.KMeansXf(torch.from_numpy(P).cuda()).cluster(start.copy())      # device points, device labels
    assert (c.getPointToClusterIndexMap() == a.getPointToClusterIndexMap()).all() and c.getClusterCentroids().tobytes() == a.getClusterCentroids().tobytes()


# ---- 7: reproducibility and limits -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kind", [("blobs5", R.NORMALIZED_RANDOM_WALK), ("shells", R.NORMALIZED_SYMMETRIC), ("uniform", R.UNNORMALIZED)])
def test_two_runs_give_the_same_bytes(name, kind):
    from cilantro_amd import clustering as cl

    planted = R.cloud(name)[1]
    runs = [cl.SpectralClustering(affinities(name), 4, True, kind, initial_centroid_indices=_first_of_each(planted) + [1, 2, 3]) for _ in range(2)]
    assert runs[0].getEmbeddedPoints().tobytes() == runs[1].getEmbeddedPoints().tobytes()
    assert runs[0].getComputedEigenValues().tobytes() == runs[1].getComputedEigenValues().tobytes()
    assert runs[0].getPointToClusterIndexMap().tobytes() == runs[1].getPointToClusterIndexMap().tobytes()
    import torch

    E, ev, _ = cl.spectral_embedding(affinities(name), 4, True, kind, on_device=True)      # the device copy-out: the same bytes
    assert E.cpu().numpy().tobytes() == runs[0].getEmbeddedPoints().tobytes()


def _raw_embedding(W, **kw):
    L = capi.load()
    prm, res = capi.SpectralParams(), capi.SpectralResult()
    L.cilhip_spectral_default_params(C.byref(prm))
    for key, v in kw.items():
        setattr(prm, key, v)
    n = W.info()[0]
    emb, ev = np.full(n * 17, 7, F32), np.full(18, 7, F32)
    rc = L.cilhip_spectral_embedding(W._h, C.byref(prm), emb.ctypes.data, ev.ctypes.data, capi.MEM_HOST, C.byref(res))
    return rc, res, emb, ev


def test_an_iteration_limit_is_reported_not_hidden():
    from cilantro_amd import clustering as cl

    rc, res, emb, ev = _raw_embedding(affinities("uniform"), max_num_clusters=3, estimate_num_clusters=1, max_outer=1)
    assert rc == capi.OK and res.num_eigenvalues == 4 and res.n_converged < 4 and res.outer_iterations == 1 and res.max_residual > 0
    with pytest.raises(capi.CilhipError, match="converged"):
        cl.spectral_embedding(affinities("uniform"), 3, True, max_outer=1)


def test_refusals_that_need_a_handle():
    from cilantro_amd import clustering as cl

    L = capi.load()
    W = affinities("blobs3")
    rc, res, emb, ev = _raw_embedding(W, max_num_clusters=17)
    assert rc == capi.ERR_UNSUPPORTED and b"16" in L.cilhip_last_error(None) and (emb == 7).all() and (ev == 7).all()
    for kw in (dict(laplacian_type=3), dict(degree=1), dict(guard=0), dict(max_outer=0)):
        rc, res, emb, ev = _raw_embedding(W, **kw)
        assert rc == capi.ERR_INVALID and b"spectral_embedding" in L.cilhip_last_error(None) and (emb == 7).all()
    rc, res, emb, ev = _raw_embedding(W, max_num_clusters=300)      # >= n: two clusters, estimation off (S3)
    assert rc == capi.OK and res.num_clusters == 2 and res.num_eigenvalues == 2
    # a row without an entry: degree 0
    lonely = cl.SparseMatrix.from_csr(4, [0, 1, 2, 2, 3], [1, 0, 3], [1.0, 1.0, 1.0])
    for kind in (1, 2):
        rc, res, emb, ev = _raw_embedding(lonely, laplacian_type=kind)
        assert rc == capi.ERR_INVALID and b"degree" in L.cilhip_last_error(None) and (emb == 7).all()
    rc, res, emb, ev = _raw_embedding(lonely, laplacian_type=0)
    assert rc == capi.OK and res.n_converged == 2
    lonely.close()
    two = cl.SparseMatrix.from_csr(2, [0, 1, 2], [1, 0], [1.0, 1.0])
    rc, res, emb, ev = _raw_embedding(two)
    assert rc == capi.ERR_INVALID and b"n < 3" in L.cilhip_last_error(None)
    two.close()


def test_nothing_stays_allocated():
    from cilantro_amd import clustering as cl

    L = capi.load()
    live = (C.c_ulonglong * 2)()
    L.cilhip_debug_live_allocations(live)
    before = tuple(live)
    idx, d2 = lists("blobs3")
    W = cl.nn_graph_sparse_matrix((idx, d2), cl.RBFKernelWeightEvaluator(1.0), True)
    L.cilhip_debug_live_allocations(live)
    assert live[0] == before[0] + 3      # offsets, columns, values
    cl.SpectralClustering(W, 4, True, initial_centroid_indices=[0, 100, 200])
    bad = idx.copy()
    bad[0, 0] = 999
    with pytest.raises(capi.CilhipError):
        cl.nn_graph_sparse_matrix((bad, d2), None, True)
    W.close()
    L.cilhip_debug_live_allocations(live)
    assert tuple(live) == before
