"""CPU: the yardstick of the spectral-clustering entries (tests/_spectral_refs.py) pinned against itself, the properties of the inputs
that tests/test_gpu_spectral.py relies on, what the entries answer before they have a device, and the host C++ parts (csrc/small_sym.hpp,
the mirror in cilantro_hip/clustering.hpp, examples/spectral_clustering.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _spectral_refs as R
from cilantro_amd import capi
from test_components_refs_cpu import build_cpp
from test_stateless_entries_cpu import NO_TEXT, _has_gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED, NO_DEVICE = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED, capi.ERR_NO_DEVICE
HOST = capi.MEM_HOST
F32 = np.float32
SMALL = ["blobs3", "blobs5", "shells", "uniform"]
COMPONENTS = {"blobs3": 3, "blobs5": 5, "shells": 2, "uniform": 1}
_graphs = {}


def graph(name):
    """the symmetric RBF (sigma 1) k-NN graph of an input, from CPU lists -> (n, offsets, columns, values)"""
    if name not in _graphs:
        P, _ = R.cloud(name)
        idx, d2 = R.knn_lists(P, R.INPUTS[name][1])
        _graphs[name] = (len(P),) + R.graph_csr(len(P), idx, d2, None, R.RBF, 1.0, True, 0)
    return _graphs[name]


def components(n, off, col):
    lab = np.arange(n)
    row = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    while True:
        new = lab.copy()
        np.minimum.at(new, row, lab[col.astype(np.int64)])
        np.minimum.at(new, col.astype(np.int64), lab[row])
        if (new == lab).all():
            return len(np.unique(lab)), lab
        lab = new


# ---- the inputs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SMALL)
def test_inputs_have_the_properties_the_gpu_tests_rely_on(name):
    n, off, col, val = graph(name)
    P, planted = R.cloud(name)
    W = R.dense(n, off, col, val)
    assert (W == W.T).all() and (W.sum(1) > 0).all()
    count, lab = components(n, off, col)
    assert count == COMPONENTS[name]
    assert all(len(np.unique(planted[lab == c])) == 1 for c in np.unique(lab))      # the components ARE the planted parts
    nev = R.INPUTS[name][2]
    A, ub, _ = R.laplacian(W, R.NORMALIZED_SYMMETRIC)
    lam = np.linalg.eigvalsh(A)
    assert (np.abs(lam[:count]) < 1e-12).all() and lam[count] > 1e-3      # a zero eigenvalue per component, then a gap
    assert lam[nev] - lam[nev - 1] > 2e-3, lam[:nev + 1]                    # the gap behind the wanted set (Davis-Kahan's delta)
    ev = np.maximum(lam[:nev].astype(F32), 0)
    assert R.eigengap(ev, nev - 1) == (count if count > 1 else 1)
    assert lam[-1] <= ub


# ---- S1: the literal loop against the vectorised builder ---------------------------------------------------------------------------------
def _same(n, M, csr):
    off, col, val = csr
    rows = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
    assert len(M) == len(col)
    assert all((np.diff(col[off[r]:off[r + 1]].astype(np.int64)) > 0).all() for r in range(n))
    got = {(int(r), int(c)): v for r, c, v in zip(rows, col, val)}
    assert got.keys() == M.keys()
    assert all(np.float32(M[k]).tobytes() == np.float32(got[k]).tobytes() for k in M)


@pytest.mark.parametrize("duplicates", [0, 1])
@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("kind", [R.UNITY, R.IDENTITY, R.RBF])
def test_literal_triplet_loop_equals_vectorised_builder(kind, sym, duplicates):
    P, _ = R.cloud("blobs3")
    idx, d2 = R.knn_lists(P, 8)
    idx = idx.copy()
    idx[5, 6:] = R.NONE      # a short list
    idx[7, 3] = idx[7, 2]    # a list that names a point twice: three values can meet on one entry
    n = len(P)
    _same(n, R.graph_literal(n, idx, d2, None, kind, 0.7, sym, duplicates), R.graph_csr(n, idx, d2, None, kind, 0.7, sym, duplicates))
    off, ci, cd = R.lists_to_csr(idx, d2)
    a, b = R.graph_csr(n, idx, d2, None, kind, 0.7, sym, duplicates), R.graph_csr(n, ci, cd, off, kind, 0.7, sym, duplicates)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))      # both list layouts


def test_forced_symmetry_doubles_mutual_pairs_and_self_entries():
    idx = np.array([[0, 1], [1, 0], [2, 0]], np.uint32)
    d2 = np.array([[0, 1], [0, 1], [0, 4]], F32)
    off, col, val = R.graph_csr(3, idx, d2, None, R.IDENTITY, 1.0, True, 0)
    W = R.dense(3, off, col, val)
    assert (W == np.array([[0, 2, 4], [2, 0, 0], [4, 0, 0]], float)).all()      # mutual pair 2 val, one-sided pair val, self 2 * 0
    off, col, val = R.graph_csr(3, idx, d2, None, R.UNITY, 1.0, True, 0)
    assert (R.dense(3, off, col, val) == np.array([[2, 2, 1], [2, 2, 0], [1, 0, 2]], float)).all()
    off, col, val = R.graph_csr(3, idx, d2, None, R.UNITY, 1.0, True, 1)
    assert (R.dense(3, off, col, val) == np.array([[1, 1, 1], [1, 1, 0], [1, 0, 1]], float)).all()      # the dense variant: assignment
    off, col, val = R.graph_csr(3, idx, d2, None, R.UNITY, 1.0, False, 0)
    assert (R.dense(3, off, col, val) == np.array([[1, 1, 1], [1, 1, 0], [0, 0, 1]], float)).all()      # M(idx, i) only


# ---- S5, S2, S6 -------------------------------------------------------------------------------------------------------------------------
def test_eigengap_on_hand_made_vectors():
    assert R.eigengap([0.25, 0.25, 0.25], 2) == 2                 # equal values: max_num_clusters
    assert R.eigengap([0.0, 0.0, 0.0, 0.5, 0.6], 4) == 3          # one gap
    assert R.eigengap([0.5, 0.6, 0.65], 2) == 1                   # every gap is below ev[0], the start value of max_diff
    assert R.eigengap([0.0, 1e-9, 0.3], 2) == 2
    assert R.eigengap([0.0, 0.0], 1) == 1


def test_random_walk_vectors_from_the_symmetric_form():
    linalg = pytest.importorskip("scipy.linalg")
    n, off, col, val = graph("blobs3")
    W = R.dense(n, off, col, val)
    A, _, d = R.laplacian(W, R.NORMALIZED_RANDOM_WALK)
    lam, U = np.linalg.eigh(A)
    V = U[:, :5] / np.sqrt(d)[:, None]
    lam_g, Vg = linalg.eigh(np.diag(d) - W, np.diag(d))
    assert np.abs(lam[:5] - lam_g[:5]).max() < 1e-12
    assert np.abs(V.T @ np.diag(d) @ V - np.eye(5)).max() < 1e-12      # v^T D v = 1
    for block in (slice(0, 3), slice(3, 5)):                             # the zero eigenvalue's space, then the two simple ones: as subspaces
        Q1, Q2 = np.linalg.qr(V[:, block])[0], np.linalg.qr(Vg[:, block])[0]
        assert np.abs(Q1 @ (Q1.T @ Q2) - Q2).max() < 1e-8


def test_kmeans_restatement_against_the_oracle_in_three_dimensions(orc):
    P, planted = R.cloud("blobs3")
    start = P[[0, 1, 250]].copy()      # two centroids start in one blob
    cent, lab, it = R.kmeans_nd(P, start, 100, R.FLT_EPS)
    oc, ol, oit = orc.kmeans(P, start, 100, R.FLT_EPS)
    assert (lab == ol).all() and it == oit
    assert (np.abs(cent - oc) <= np.spacing(np.abs(oc))).all()      # (the oracle's mode 1 sums in f64 too, in one run instead of chunks)


def test_kmeans_restatement_repairs_an_empty_cluster():
    x = np.array([[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 0], [40, 40, 40, 40, 40]], F32)
    start = np.array([[0, 0, 0, 0, 0], [50, 50, 50, 50, 50], [60, 60, 60, 60, 60]], F32)      # cluster 2 starts empty
    cent, lab, it = R.kmeans_nd(x, start, 1, 0.0)
    assert lab.tolist() == [0, 2, 0, 1]      # the farthest member of the largest cluster (lowest index among equals) moves to cluster 2 ...
    assert (cent[2] == 0).all()              # ... whose sum does not get it (kmeans.hpp:171-175)
    assert (cent[0] == np.array([0, 0.5, 0, 0, 0], F32)).all()


# ---- the entries before they have a device ----------------------------------------------------------------------------------------------
SENTINEL = 0xA5A5A5A5


def _lists(n=6, k=3):
    idx = np.stack([(np.arange(n) + j) % n for j in range(k)], 1).astype(np.uint32)
    return idx, np.ones((n, k), F32)


def graph_call(L, n=6, k=3, null=(), kind=2, sigma=1.0, mem=HOST, sym=1, duplicates=0, out=True, csr=False, device=0):
    idx, d2 = _lists(min(n, 6) or 6, min(k, 3) or 3)
    off = np.arange(7, dtype=np.uint64) * 3
    p = dict(idx=idx.ctypes.data, d2=d2.ctypes.data, off=off.ctypes.data if csr else None)
    for key in null:
        p[key] = None
    h = C.c_void_p(SENTINEL)
    rc = L.cilhip_nn_graph_matrix(device, n, p["off"], p["idx"], p["d2"], 18 if csr and k == 3 else k, mem, kind, C.c_float(sigma), sym, duplicates, C.byref(h) if out else None)
    return rc, h.value


GRAPH_REFUSED = [dict(out=False), dict(null=("idx",)), dict(null=("d2",)), dict(null=("d2",), kind=1), dict(kind=3), dict(kind=-1), dict(sigma=0.0), dict(sigma=float("nan")),
                 dict(sigma=float("inf")), dict(mem=2), dict(mem=-1), dict(duplicates=2), dict(n=0), dict(n=0xFFFFFFF0), dict(k=0), dict(n=1 << 20, k=1 << 12),
                 dict(csr=True, k=1 << 31)]


@pytest.mark.parametrize("change", GRAPH_REFUSED, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_graph_refusals(hip_lib, change):
    rc, h = graph_call(hip_lib, **change)
    assert rc == INVALID and h == SENTINEL
    assert b"nn_graph_matrix" in hip_lib.cilhip_last_error(None)


def csr_call(L, n=3, off=(0, 2, 3, 4), col=(0, 2, 1, 0), val=(1.0, 2.0, 3.0, 4.0), null=(), mem=HOST, out=True):
    a = dict(off=np.array(off, np.uint64), col=np.array(col, np.uint32), val=np.array(val, F32))
    p = {k: (None if k in null else v.ctypes.data) for k, v in a.items()}
    h = C.c_void_p(SENTINEL)
    rc = L.cilhip_sparse_from_csr(0, n, p["off"], p["col"], p["val"], mem, C.byref(h) if out else None)
    return rc, h.value


CSR_REFUSED = [(dict(out=False), b"NULL"), (dict(null=("off",)), b"NULL"), (dict(null=("col",)), b"NULL"), (dict(null=("val",)), b"NULL"), (dict(mem=2), b"mem"), (dict(n=0), b"n must"),
               (dict(col=(2, 0, 1, 0)), b"ascending"), (dict(col=(0, 0, 1, 0)), b"ascending"), (dict(col=(0, 3, 1, 0)), b"below n"),
               (dict(val=(1.0, float("nan"), 3.0, 4.0)), b"finite"), (dict(val=(1.0, 2.0, float("inf"), 4.0)), b"finite"), (dict(off=(1, 2, 3, 4)), b"offsets"),
               (dict(off=(0, 3, 2, 4)), b"offsets")]


@pytest.mark.parametrize("row", CSR_REFUSED, ids=lambda r: ",".join("%s=%s" % kv for kv in r[0].items()))
def test_from_csr_refusals(hip_lib, row):
    change, word = row
    rc, h = csr_call(hip_lib, **change)
    assert rc == INVALID and h == SENTINEL
    text = hip_lib.cilhip_last_error(None)
    assert b"sparse_from_csr" in text and word in text, text


def nd_call(L, n=8, dim=5, k=2, mem=HOST, null=(), device=0):
    rows = min(max(n, 1), 8)      # (a refused n is never read)
    a = dict(x=np.arange(rows * max(min(dim, 16), 1), dtype=F32), cent=np.full(16 * 4, 7, F32), labels=np.full(rows, SENTINEL, np.uint32))
    p = {key: (None if key in null else v.ctypes.data) for key, v in a.items()}
    it = C.c_size_t(SENTINEL)
    rc = L.cilhip_kmeans_nd(device, p["x"], n, dim, mem, p["cent"], k, 5, C.c_float(0.0), p["labels"], C.byref(it))
    untouched = (a["cent"] == 7).all() and (a["labels"] == SENTINEL).all() and it.value == SENTINEL
    return rc, untouched


@pytest.mark.parametrize("change", [dict(null=("x",)), dict(null=("cent",)), dict(n=0), dict(n=0xFFFFFFF0), dict(dim=0), dict(dim=17), dict(k=0), dict(mem=2)], ids=str)
def test_kmeans_nd_refusals(hip_lib, change):
    rc, untouched = nd_call(hip_lib, **change)
    assert rc == INVALID and untouched and b"kmeans_nd" in hip_lib.cilhip_last_error(None)


def test_kmeans_nd_above_256_clusters_is_unsupported(hip_lib):
    rc, untouched = nd_call(hip_lib, k=257)
    assert rc == UNSUPPORTED and untouched and b"kmeans_nd" in hip_lib.cilhip_last_error(None)


def test_entries_that_take_a_handle_refuse_null(hip_lib):
    v = [C.c_size_t(7) for _ in range(3)]
    assert hip_lib.cilhip_sparse_info(None, *[C.byref(x) for x in v]) == INVALID and [x.value for x in v] == [7, 7, 7]
    assert b"sparse_info" in hip_lib.cilhip_last_error(None)
    out = np.full(4, 7, np.uint64)
    assert hip_lib.cilhip_sparse_get(None, out.ctypes.data, None, None, HOST) == INVALID and (out == 7).all() and b"sparse_get" in hip_lib.cilhip_last_error(None)
    prm, res = capi.SpectralParams(), capi.SpectralResult()
    hip_lib.cilhip_spectral_default_params(C.byref(prm))
    emb, ev = np.full(8, 7, F32), np.full(4, 7, F32)
    res.num_clusters = 7
    assert hip_lib.cilhip_spectral_embedding(None, C.byref(prm), emb.ctypes.data, ev.ctypes.data, HOST, C.byref(res)) == INVALID
    assert b"spectral_embedding" in hip_lib.cilhip_last_error(None) and (emb == 7).all() and (ev == 7).all() and res.num_clusters == 7
    hip_lib.cilhip_sparse_destroy(None)      # (ignored)


def test_without_a_device_the_entries_answer_no_device(hip_lib):
    if _has_gpu():
        pytest.skip("a GPU is present")
    for call, kw in ((graph_call, dict()), (graph_call, dict(csr=True)), (graph_call, dict(kind=0, null=("d2",))), (csr_call, dict())):
        rc, h = call(hip_lib, **kw)
        assert rc == NO_DEVICE and h == SENTINEL and b"device" in hip_lib.cilhip_last_error(None)
    rc, untouched = nd_call(hip_lib)
    assert rc == NO_DEVICE and untouched and b"kmeans_nd" in hip_lib.cilhip_last_error(None)
    from cilantro_amd import clustering

    with pytest.raises(capi.CilhipError):
        clustering.SpectralClustering(np.eye(4, dtype=F32), 2)


def test_default_params_are_the_reference_literals(hip_lib):
    p = capi.SpectralParams(7, 7, 7, 7, 7, 7)
    hip_lib.cilhip_spectral_default_params(C.byref(p))
    # spectral_clustering.hpp:399-401 (NORMALIZED_RANDOM_WALK, no estimation), :204 (max_iter 1000); the filter's degree and guard: DESIGN 18
    assert (p.max_num_clusters, p.estimate_num_clusters, p.laplacian_type, p.max_outer, p.degree, p.guard) == (2, 0, 2, 1000, 24, 3)
    hip_lib.cilhip_spectral_default_params(None)      # (ignored)
    from cilantro_amd import clustering

    assert (clustering.GraphLaplacianType.UNNORMALIZED, clustering.GraphLaplacianType.NORMALIZED_SYMMETRIC, clustering.GraphLaplacianType.NORMALIZED_RANDOM_WALK) == (0, 1, 2)
    assert R.TOL == float(F32(1e-7)) and abs(R.EPS23 - R.FLT_EPS ** (2 / 3)) < 1e-9


def test_symbols_present():
    names = ["cilhip_nn_graph_matrix", "cilhip_sparse_from_csr", "cilhip_sparse_info", "cilhip_sparse_get", "cilhip_sparse_destroy", "cilhip_spectral_default_params",
             "cilhip_spectral_embedding", "cilhip_kmeans_nd"]
    raw = C.CDLL(capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")).read()
    assert all(n in capi.SYMBOLS and hasattr(raw, n) and n + "(" in header for n in names)
    from cilantro_amd import build

    assert "spectral.hip" in build.SOURCES and "small_sym.hpp" in build.HEADERS


# ---- host C++ ------------------------------------------------------------------------------------------------------------------------------
def test_small_sym_on_host(tmp_path):
    """csrc/small_sym.hpp (Jacobi, Cholesky, triangular inverse) on random, repeated-eigenvalue and 1 x 1 matrices; once more as a
    stand-alone program under the address and undefined-behaviour sanitizers"""
    src = os.path.join(ROOT, "tests", "cpp", "test_small_sym.cpp")
    for flags, name in ((["-O2"], "test_small_sym"), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_small_sym_san")):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def test_cpp_mirror_and_example_compile():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_spectral.cpp"), "test_spectral")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    example = build_cpp(os.path.join(ROOT, "examples", "spectral_clustering.cpp"), "example_spectral_clustering")
    r = subprocess.run([example, "--describe"], capture_output=True, text=True)
    assert r.returncode == 0 and "Number of points: 1700" in r.stdout
