"""No GPU: the yardstick of DESIGN.md section 19 itself (tests/_mds_refs.py), the plain-C++ helpers of the solver, and everything the
multidimensional-scaling and principal-component entries decide before they need a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _mds_refs as R
from cilantro_amd import capi
from test_components_refs_cpu import build_cpp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
NEW = ["cilhip_mds_default_params", "cilhip_mds_embedding", "cilhip_mds_apply", "cilhip_pca_fit", "cilhip_pca_project", "cilhip_pca_reconstruct"]


def test_embedding_dimension_on_hand_made_vectors():
    assert R.embedding_dim([500.0, 500.0, 5.0, 0.0], 3) == 2       # the largest drop follows the second value
    assert R.embedding_dim([9.0, 1.0, 0.5], 2) == 1
    assert R.embedding_dim([4.0, 3.0, 0.0], 2) == 2
    assert R.embedding_dim([2.0, 2.0, 2.0, 2.0], 3) == 3             # all equal: max_dim (:29)
    assert R.embedding_dim([1.0], 5) == 5
    assert R.embedding_dim([1.0, 1.0, 1.0 + R.FLT_EPS], 2) == 1      # a spread of exactly epsilon is not below epsilon; drops 0, -eps: the first
    from cilantro_amd.multidimensional_scaling import estimateEmbeddingDimensionEigengap as mirror

    rng = np.random.default_rng(0)
    for _ in range(50):
        ev = np.sort(rng.random(rng.integers(1, 8)).astype(F32))[::-1]
        assert mirror(ev, 4) == R.embedding_dim(ev, 4)


def test_sizes():
    assert R.sizes(1000, 2, False) == (2, False, 2) and R.sizes(1000, 3, True) == (3, True, 4)
    assert R.sizes(4, 3, True) == (3, True, 3) and R.sizes(10, 0, True) == (2, False, 2) and R.sizes(10, 10, True) == (2, False, 2)


def test_centred_matrix_of_a_euclidean_cloud_is_its_gram_matrix():
    P = np.random.default_rng(1).standard_normal((40, 3))
    Pc = P - P.mean(0)
    assert np.abs(R.centred(R.sqdist(P).astype(F64)) - Pc @ Pc.T).max() <= 40 * np.finfo(F32).eps * R.sqdist(P).max()
    assert R.squared(np.full((2, 2), 3.0, F32), False)[0, 0] == 9.0


@pytest.mark.parametrize("name", list(R.INPUTS))
def test_the_model_of_the_solver_converges_on_every_input_of_the_gpu_tests(name):
    D = R.matrix(name)[0]
    lam, _, norm = R.spectrum(name)
    for max_dim, estimate in R.INPUTS[name][1]:
        r = R.solve(D, max_dim, estimate)
        print(name, max_dim, estimate, {k: r[k] for k in ("nev", "n_converged", "outer", "products", "residual")})
        assert r["n_converged"] == r["nev"]
        assert (np.abs(np.abs(r["theta"]) - np.abs(lam[:r["nev"]])) <= R.eigenvalue_bound(lam[:r["nev"]], len(D), norm)).all()


def test_the_model_gives_up_on_a_pair_inside_the_rounding_noise():
    """the circle has rank 3: (3, true) asks for a fourth pair among the +-1e-5 eigenvalues the f32 rounding of the distances leaves"""
    r = R.solve(R.matrix("circle")[0], 3, True, max_outer=5)
    print({k: r[k] for k in ("nev", "n_converged", "outer", "theta")})
    assert r["nev"] == 4 and r["n_converged"] < 4 and r["outer"] == 5


def test_filter_plan_of_the_model():
    assert R.filter_plan(500.0, 1e-5, 500.0, 0.0, 24) == (1e-5, 24)
    assert R.filter_plan(100.0, 1.0, 1.0, 0.0, 24) == (1.0, 2)
    assert R.filter_plan(0.5, 0.5, 0.5, 0.0, 24) == (0.25, 24)
    e, m = R.filter_plan(4.0, 1.0, 4.0, 480.0, 24)
    assert e == 1.0 and m == int(np.floor(np.log(1e10) / (np.arccosh(480.0) - np.arccosh(4.0))))


def test_mds_host_helpers(tmp_path):
    """csrc/mds_host.hpp alone; once more as a stand-alone program under the address and undefined-behaviour sanitizers"""
    src = os.path.join(ROOT, "tests", "cpp", "test_mds_host.cpp")
    for flags, name in ((["-O2"], "test_mds_host"), (["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "test_mds_host_san")):
        exe = str(tmp_path / name)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-ffp-contract=off"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ALL OK" in r.stdout, r.stdout + r.stderr


def test_pca_restatement():
    x = (1e3 + np.random.default_rng(2).standard_normal((300, 3)) * [2.0, 1.0, 0.5]).astype(F32)
    mean, cov, valid = R.pca_moments(x)
    assert valid and np.abs(mean - x.astype(F64).mean(0)).max() <= 1e3 * np.finfo(F32).eps
    assert np.abs(cov - np.cov(x.astype(F64).T)).max() <= 4.0 * 4 * np.finfo(F32).eps      # (x - mean rounded at 1e3: 6e-5 on a spread of 2)
    lam, Q = R.pca_eigen(cov)
    assert (np.diff(lam) <= 0).all() and np.linalg.det(Q) > 0 and np.abs(Q @ Q.T - np.eye(3)).max() <= 1e-14
    for c in range(2):
        assert Q[c].max() == np.abs(Q[c]).max()
    assert not R.pca_moments(x[:1])[2] and np.isnan(R.pca_moments(x[:1])[0]).all()
    m2, c2, _ = R.pca_moments(x, [5, 7, 7, 200])
    assert np.abs(m2 - x[[5, 7, 7, 200]].astype(F64).mean(0)).max() <= 1e3 * np.finfo(F32).eps
    y = R.project(x, mean, Q, 3)
    assert np.abs(R.reconstruct(y, mean, Q) - x).max() <= 1e3 * 4 * np.finfo(F32).eps
    assert R.project(x, mean, Q, 2).shape == (300, 2) and R.reconstruct(y[:, :2], mean, Q).shape == (300, 3)


def test_new_symbols_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")).read()
    L = capi.load()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in capi.SYMBOLS and getattr(L, name) is not None
    assert "multidimensional scaling" not in header.split("cilhip_nn_graph_matrix(")[0].split("Not built")[-1]


def _mds(D, n, mem=capi.MEM_HOST, prm=None, emb=True, ev=True, res=True):
    L = capi.load()
    p = capi.MdsParams()
    L.cilhip_mds_default_params(C.byref(p))
    for k, v in (prm or {}).items():
        setattr(p, k, v)
    out, evs, r = np.full(64, 7.0, F32), np.full(20, 7.0, F32), capi.MdsResult()
    rc = L.cilhip_mds_embedding(0, None if D is None else D.ctypes.data, n, mem, C.byref(p) if prm is not False else None, out.ctypes.data if emb else None,
                                evs.ctypes.data if ev else None, C.byref(r) if res else None)
    assert (out == 7.0).all() and (evs == 7.0).all()      # the outputs are untouched
    return rc, L.cilhip_last_error(None).decode()


def test_argument_errors_are_refused_before_any_device_call():
    L = capi.load()
    p = capi.MdsParams()
    L.cilhip_mds_default_params(C.byref(p))
    assert (p.max_dim, p.estimate_dim, p.distances_are_squared, p.max_outer, p.degree, p.guard) == (2, 0, 1, 1000, 24, 3)
    D = np.zeros((4, 4), F32)
    for kw in (dict(D=None, n=4), dict(D=D, n=4, prm=False), dict(D=D, n=4, emb=False), dict(D=D, n=4, ev=False), dict(D=D, n=4, res=False)):
        rc, msg = _mds(**kw)
        assert rc == capi.ERR_INVALID and "M1" in msg and "NULL" in msg, msg
    for n in (0, 2, 2 ** 32 - 16, 2 ** 40):
        rc, msg = _mds(D, n)
        assert rc == capi.ERR_INVALID and "M1" in msg and "n must lie" in msg, msg
    rc, msg = _mds(D, 4, mem=2)
    assert rc == capi.ERR_INVALID and "mem" in msg
    for prm in (dict(degree=0), dict(degree=513), dict(guard=0), dict(guard=16), dict(max_outer=0)):
        assert _mds(D, 4, prm=prm)[0] == capi.ERR_INVALID
    rc, msg = _mds(np.zeros((32, 32), F32), 32, prm=dict(max_dim=17))      # M3
    assert rc == capi.ERR_UNSUPPORTED and "M3" in msg, msg
    y = np.zeros(8)
    assert L.cilhip_mds_apply(0, D.ctypes.data, 4, capi.MEM_HOST, 1, y.ctypes.data, 33, y.ctypes.data, None) == capi.ERR_INVALID
    assert L.cilhip_mds_apply(0, D.ctypes.data, 2, capi.MEM_HOST, 1, y.ctypes.data, 1, y.ctypes.data, None) == capi.ERR_INVALID
    # PCA
    x, out, valid = np.zeros((4, 3), F32), np.zeros(16 * 16, F32), C.c_int(5)
    fit = lambda n, dim, mem=capi.MEM_HOST, xp=x.ctypes.data: L.cilhip_pca_fit(0, xp, n, dim, None, 0, mem, out.ctypes.data, out.ctypes.data, out.ctypes.data, out.ctypes.data, C.byref(valid))
    assert fit(4, 0) == fit(4, 17) == fit(0, 3) == fit(4, 3, 2) == fit(4, 3, xp=None) == capi.ERR_INVALID and valid.value == 5
    assert L.cilhip_pca_project(0, x.ctypes.data, 4, 3, capi.MEM_HOST, out.ctypes.data, out.ctypes.data, 4, out.ctypes.data) == capi.ERR_INVALID      # P5: target_dim > dim
    assert "P5" in L.cilhip_last_error(None).decode()
    assert L.cilhip_pca_reconstruct(0, x.ctypes.data, 4, 4, 3, capi.MEM_HOST, out.ctypes.data, out.ctypes.data, out.ctypes.data) == capi.ERR_INVALID
    assert L.cilhip_pca_project(0, x.ctypes.data, 4, 3, capi.MEM_HOST, None, out.ctypes.data, 2, out.ctypes.data) == capi.ERR_INVALID


def test_cpp_mirrors_and_examples_compile():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_mds_pca.cpp"), "test_mds_pca")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    build_cpp(os.path.join(ROOT, "examples", "multidimensional_scaling.cpp"), "example_multidimensional_scaling")
    build_cpp(os.path.join(ROOT, "examples", "principal_component_analysis.cpp"), "example_principal_component_analysis")
    src = open(os.path.join(ROOT, "examples", "multidimensional_scaling.cpp")).read()
    for needle in ("MultidimensionalScaling<float, 2> mds(", "num_points = 1000", "0.1f * std::sin(10.0f"):
        assert needle in src, needle
