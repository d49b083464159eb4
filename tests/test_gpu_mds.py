"""GPU: cilhip_mds_embedding / cilhip_mds_apply and their Python / C++ mirrors against tests/_mds_refs.py -- DESIGN.md section 19, rules M1-M5 of
c_api.h.  Eigenpairs are compared with dense f64 numpy.linalg.eigh of -1/2 J Dhat J of the same f32-valued matrix.  Every bound is derived
where it is used; each test prints its figures before it asserts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _mds_refs as R
from cilantro_amd import capi
from test_components_refs_cpu import build_cpp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64
EPS32, EPS64 = float(np.finfo(F32).eps), float(np.finfo(F64).eps)
REQUESTS = [(name, md, est) for name, (_, reqs) in R.INPUTS.items() for md, est in reqs]
_cache = {}


def run(name, max_dim, estimate, **kw):
    from cilantro_amd import multidimensional_scaling as mds

    key = (name, max_dim, estimate, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = mds.mds_embedding(R.matrix(name)[0], max_dim, estimate, **kw)
    return _cache[key]


# ---- 1: the operator (M1, M2) -------------------------------------------------------------------------------------------------------
def _operator_case(D, b, squared=True, on_device=False, seed=0):
    from cilantro_amd import multidimensional_scaling as mds

    n = len(D)
    X = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, b))
    Dhat = R.squared(D, squared)
    want = R.centred(Dhat) @ X
    if on_device:
        import torch

        got = mds.mds_apply(torch.from_numpy(D).cuda(), torch.from_numpy(X).cuda(), squared)[0].cpu().numpy()
    else:
        got = mds.mds_apply(D, X, squared)[0]
    # (B x)_i is four sums of at most n terms, each term at most max Dhat * max |x| = max Dhat, and n more inside every mean: a sum of n
    # terms is off by at most n eps64 times the sum of their magnitudes, on the device and in numpy alike
    bound = 8.0 * n * n * EPS64 * float(Dhat.max())
    err = float(np.abs(got - want).max())
    print(f"n {n} b {b} squared {squared} device {on_device}: max error {err:.3e} bound {bound:.3e} scale {np.abs(want).max():.3e}")
    assert err <= bound
    return got


# the widths take every compiled form (1, 4, 8, 12, 16, 24, 32 columns); the sizes lie around the 128-row chunk, its 64-row tile and the
# 256- and 1024-column blocks of the 4- and 16-byte loads (n % 4 == 0: 16 bytes per lane up to 16 columns)
@pytest.mark.parametrize("name", ["gauss5_3", "gauss5_63", "gauss5_64", "gauss5_65", "edge_127", "edge_128", "edge_129", "edge_255", "edge_256", "gauss5_257", "edge_1023", "edge_1024",
                                  "edge_1025", "edge_1028"])
def test_operator_around_every_edge(name):
    D = R.matrix(name)[0]
    for b in (1, 5):
        _operator_case(D, b)


@pytest.mark.parametrize("b", [1, 2, 4, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32])
@pytest.mark.parametrize("name", ["edge_256", "gauss5_257"])
def test_operator_at_every_width(name, b):
    _operator_case(R.matrix(name)[0], b)


def test_operator_on_distances_that_are_not_squared_and_on_device_memory():
    D = np.sqrt(R.matrix("edge_256")[0]).astype(F32)
    a = _operator_case(D, 5, squared=False)
    b = _operator_case(D, 5, squared=False, on_device=True)
    assert a.tobytes() == b.tobytes()
    D = np.sqrt(R.matrix("gauss5_257")[0]).astype(F32)
    assert _operator_case(D, 3, squared=False).tobytes() == _operator_case(D, 3, squared=False, on_device=True).tobytes()


@pytest.mark.parametrize("n", [510, 511, 512, 514])
def test_operator_around_the_column_block_of_the_wide_form(n):
    """above 16 columns a lane owns 2 matrix columns (8-byte loads, even n): a block of 256 lanes covers 512"""
    _operator_case(R.gauss5(n)[0], 17)


def test_operator_past_the_size_where_the_chunks_grow():
    """above 8192 rows a chunk holds ceil(n / 64) rows instead of 128: 8260 rows make 64 chunks of 130 = 64 + 64 + 2 rows, the last one shorter"""
    _operator_case(R.gauss5(8260)[0], 3)


@pytest.mark.parametrize("b", [5, 17])
def test_operator_does_not_depend_on_the_load_width(b):
    """a device matrix at an address that is no multiple of 16 (8) takes the narrower loads: the same bits as the widest form"""
    import torch

    from cilantro_amd import multidimensional_scaling as mds

    D = R.matrix("edge_256")[0]
    X = np.random.default_rng(1).uniform(-1.0, 1.0, (256, b))
    want = mds.mds_apply(D, X)[0].tobytes()
    for shift in (1, 2):
        buf = torch.empty(256 * 256 + shift, dtype=torch.float32, device="cuda")
        buf[shift:] = torch.from_numpy(D).reshape(-1).cuda()
        shifted = buf[shift:].view(256, 256)
        assert shifted.data_ptr() % 16 == 4 * shift
        assert mds.mds_apply(shifted, torch.from_numpy(X).cuda())[0].cpu().numpy().tobytes() == want


# ---- 2: eigenvalues (M3, M4, M5) -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_dim,estimate", REQUESTS)
def test_eigenvalues(name, max_dim, estimate):
    D = R.matrix(name)[0]
    n = len(D)
    lam, _, norm = R.spectrum(name)
    emb, ev, info = run(name, max_dim, estimate)
    dim, est, nev = R.sizes(n, max_dim, estimate)
    print(f"{name} ({max_dim}, {estimate}): {info}")
    assert info["num_eigenvalues"] == nev == len(ev) and info["n_converged"] == nev
    want = lam[:nev]
    # Weyl on the accepted residual + the rounding to f32 + the yardstick's own error
    bound = R.eigenvalue_bound(want, n, norm)
    err = np.abs(ev.astype(F64) - np.maximum(want, 0.0))
    print("eigenvalues", ev, "reference", want, "error", err, "bound", bound)
    assert (err <= bound).all()
    assert (ev[want < -bound] == 0).all() and (ev >= 0).all()
    pos = ev[want > 0]
    assert (np.diff(pos) <= 0).all(), "magnitude order"
    assert emb.shape == (n, info["dim"]) and emb.dtype == F32
    if est:
        assert info["dim"] == R.embedding_dim(ev, dim)
    else:
        assert info["dim"] == dim


@pytest.mark.parametrize("name,max_dim,estimate", REQUESTS)
def test_every_column_is_an_eigenvector(name, max_dim, estimate):
    """the returned column, normalised in f64, against the dense operator: the accepted residual, plus what the f32 rounding of the column
    (two roundings of half an ulp per entry: eps32 in norm, and as much again from normalising) and of the eigenvalue (half an ulp) add"""
    D = R.matrix(name)[0]
    B = R.centred(D)
    lam, _, norm = R.spectrum(name)
    emb, ev, info = run(name, max_dim, estimate)
    for c in range(info["dim"]):
        y = emb[:, c].astype(F64)
        if ev[c] == 0:
            assert (emb[:, c] == 0).all()      # a clamped (negative) eigenvalue: the column is zero
            continue
        assert emb[:, c].max() == np.abs(emb[:, c]).max(), "sign rule"
        x = y / np.linalg.norm(y)
        res = float(np.linalg.norm(B @ x - float(ev[c]) * x))
        bound = float(R.criterion(ev[c])) + (norm + float(ev[c])) * 2.0 * EPS32 + 0.5 * float(R.ulp32(ev[c])) + len(D) * EPS64 * norm
        print(f"{name} column {c}: eigenvalue {ev[c]:.8g} residual {res:.3e} bound {bound:.3e}")
        assert res <= bound
        # sqrtf(ev) scaling: the column's norm is sqrt(ev) up to the f32 roundings of the entries and of the root
        assert abs(np.linalg.norm(y) - np.sqrt(float(ev[c]))) <= 4.0 * EPS32 * np.sqrt(float(ev[c]))


@pytest.mark.parametrize("name,max_dim", [("gauss5_257", 4), ("wavy_sheet", 3), ("cloud3", 3), ("negative", 3), ("gauss40_decay", 16)])
def test_simple_eigenvalues_give_the_reference_vectors(name, max_dim):
    lam, Q, norm = R.spectrum(name)
    emb, ev, info = run(name, max_dim, False)
    n = len(Q)
    for c in range(info["dim"]):
        if lam[c] <= 0:
            continue
        gap = float(np.min(np.abs(np.delete(lam, c) - lam[c])))
        ref = np.sqrt(lam[c]) * Q[:, c]
        y = emb[:, c].astype(F64)
        if y @ ref < 0:
            ref = -ref
        # Davis-Kahan: sin(angle) <= residual / gap, ||x - v|| <= sqrt(2) sin; the yardstick's vector is off by n eps64 ||B|| / gap; the
        # scale differs by the eigenvalue's error; f32 rounding of root and entries
        sin = (float(R.criterion(lam[c])) + n * EPS64 * norm) / gap
        bound = np.sqrt(lam[c]) * (np.sqrt(2.0) * sin + 4.0 * EPS32) + float(R.eigenvalue_bound(lam[c], n, norm)) / (2.0 * np.sqrt(lam[c]))
        err = float(np.linalg.norm(y - ref))
        print(f"{name} column {c}: lambda {lam[c]:.6g} gap {gap:.3g} error {err:.3e} bound {bound:.3e}")
        assert err <= bound


@pytest.mark.parametrize("name,max_dim", [("circle", 2), ("circle", 3), ("ring", 2), ("gauss40_iso", 3)])
def test_degenerate_groups_give_the_reference_gram_matrix(name, max_dim):
    """Y Y^T = P_X B P_X against P_Q B P_Q of the reference: 2 ||B|| ||P_X - P_Q||, and the sin-theta theorem bounds the projectors' distance
    by ||R||_F / gap with the gap at the cut"""
    lam, Q, norm = R.spectrum(name)
    emb, ev, info = run(name, max_dim, False)
    n, dim = len(Q), info["dim"]
    gap = float(abs(lam[dim - 1]) - abs(lam[dim]))
    ref = (Q[:, :dim] * lam[:dim][None, :]) @ Q[:, :dim].T
    Y = emb.astype(F64)
    res = np.sqrt(dim) * float(R.criterion(lam[0]))
    bound = 2.0 * norm * (res + n * EPS64 * norm) / gap + dim * float(R.eigenvalue_bound(lam[0], n, norm)) + 8.0 * EPS32 * norm
    err = float(np.linalg.norm(Y @ Y.T - ref, 2))
    print(f"{name} dim {dim}: gap at the cut {gap:.4g} error {err:.3e} bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("name", ["circle", "cloud3", "wavy_sheet"])
def test_euclidean_distances_are_reproduced(name):
    """rank <= 3: Y Y^T differs from B by the part of the spectrum left out (|lambda_4|, the rounding noise of the f32 matrix) and by the
    subspace's error as above; a squared distance is B_ii + B_jj - 2 B_ij: four entries"""
    D = R.matrix(name)[0]
    lam, Q, norm = R.spectrum(name)
    emb, ev, info = run(name, 3, False)
    n = len(D)
    gap = float(lam[2] - abs(lam[3]))
    inner = 2.0 * norm * (np.sqrt(3.0) * float(R.criterion(lam[0])) + n * EPS64 * norm) / gap + abs(lam[3]) + 3.0 * float(R.eigenvalue_bound(lam[0], n, norm)) + 8.0 * EPS32 * norm
    Y = emb.astype(F64)
    g = Y @ Y.T
    d = np.diag(g)[:, None] + np.diag(g)[None, :] - 2.0 * g
    err = float(np.abs(d - D.astype(F64)).max())
    print(f"{name}: largest distance error {err:.3e} bound {4.0 * inner:.3e} (largest distance {D.max():.3g})")
    assert err <= 4.0 * inner


def test_the_ring_clamps_its_negative_third_value():
    emb, ev, info = run("ring", 2, True)
    lam = R.spectrum("ring")[0]
    print("ring eigenvalues", ev, "reference", lam[:3], info)
    assert lam[2] < 0 and ev[2] == 0 and info["num_eigenvalues"] == 3
    assert info["dim"] == R.embedding_dim(ev, 2)
    full = run("ring", 3, False)
    assert full[1][2] == 0 and (full[0][:, 2] == 0).all()


def test_distances_that_are_not_squared():
    from cilantro_amd import multidimensional_scaling as mds

    D = np.sqrt(R.matrix("gauss5_65")[0]).astype(F32)
    B = R.centred(R.squared(D, False))
    lam = np.linalg.eigvalsh(B)
    lam = lam[np.argsort(-np.abs(lam))][:4]
    emb, ev, info = mds.mds_embedding(D, 4, distances_are_squared=False)
    bound = R.eigenvalue_bound(lam, 65, float(np.abs(lam).max()))
    print("eigenvalues", ev, "reference", lam, "bound", bound)
    assert (np.abs(ev - lam) <= bound).all()


# ---- 3: memory, reproducibility, refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,max_dim,estimate", [("gauss5_64", 4, False), ("gauss5_257", 4, False), ("ring", 2, True)])
def test_host_and_device_memory_and_two_runs_give_the_same_bytes(name, max_dim, estimate):
    import torch

    from cilantro_amd import multidimensional_scaling as mds

    D = R.matrix(name)[0]
    a = mds.mds_embedding(D, max_dim, estimate)
    b = mds.mds_embedding(D, max_dim, estimate)
    c = mds.mds_embedding(torch.from_numpy(D).cuda(), max_dim, estimate)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert c[0].is_cuda and a[0].tobytes() == c[0].cpu().numpy().tobytes() and a[1].tobytes() == c[1].tobytes()
    for k in ("dim", "n_converged", "outer_iterations", "block_products", "locked"):
        assert a[2][k] == b[2][k] == c[2][k]


def _live():
    out = (C.c_ulonglong * 2)()
    assert capi.load().cilhip_debug_live_allocations(out) == capi.OK
    return out[0], out[1]


def test_non_finite_entries_are_refused_and_nothing_stays_allocated():
    from cilantro_amd import multidimensional_scaling as mds

    before = _live()
    L = capi.load()
    for bad in (np.nan, np.inf, -np.inf):
        D = R.matrix("gauss5_65")[0].copy()
        D[40, 17] = D[17, 40] = bad
        prm = capi.MdsParams()
        L.cilhip_mds_default_params(C.byref(prm))
        emb, ev, res = np.full((65, 2), 7.0, F32), np.full(3, 7.0, F32), capi.MdsResult()
        rc = L.cilhip_mds_embedding(0, D.ctypes.data, 65, capi.MEM_HOST, C.byref(prm), emb.ctypes.data, ev.ctypes.data, C.byref(res))
        msg = L.cilhip_last_error(None).decode()
        print(bad, rc, msg)
        assert rc == capi.ERR_INVALID and "M1" in msg and (emb == 7.0).all() and (ev == 7.0).all()
    mds.mds_embedding(R.matrix("gauss5_65")[0], 2)
    assert _live() == before


def test_an_iteration_limit_is_reported_not_hidden():
    """the documented case: the circle has rank 3, so (3, true) asks for a fourth pair inside the +-1e-5 rounding eigenvalues"""
    from cilantro_amd import multidimensional_scaling as mds

    D = R.matrix("circle")[0]
    emb, ev, info = mds.mds_embedding(D, 3, True, max_outer=5, raise_unconverged=False)
    print(info, ev)
    assert info["num_eigenvalues"] == 4 and info["n_converged"] < 4 and info["outer_iterations"] == 5
    with pytest.raises(capi.CilhipError):
        mds.mds_embedding(D, 3, True, max_outer=5)


def test_the_mirror_classes():
    from cilantro_amd import multidimensional_scaling as mds

    D = R.matrix("cloud3")[0]
    m3 = mds.MultidimensionalScaling3f(D)
    mx = mds.MultidimensionalScalingXf(D, 3)
    assert m3.getEmbeddingDimension() == 3 and m3.getEmbeddedPoints().tobytes() == mx.getEmbeddedPoints().tobytes()
    assert mds.MultidimensionalScaling2f(D).getEmbeddedPoints().shape == (300, 2)
    assert mds.MultidimensionalScaling(D, 0).getEmbeddingDimension() == 2 and mds.MultidimensionalScaling(D, 300, True).getEmbeddingDimension() == 2      # M3's fall-back
    est = mds.MultidimensionalScaling(D, 2, True)      # (max_dim below the cloud's rank, 3: the extra pair is a real one)
    ev = est.getComputedEigenValues()
    assert len(ev) == 3 and est.getEmbeddingDimension() == mds.estimateEmbeddingDimensionEigengap(ev, 2) == R.embedding_dim(ev, 2)


# ---- 4: the C++ mirror and the examples -----------------------------------------------------------------------------------------------
def test_cpp_mirror_and_examples():
    exe = build_cpp(os.path.join(ROOT, "tests", "cpp", "test_mds_pca.cpp"), "test_mds_pca")
    r = subprocess.run([exe, "run"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
    ex = build_cpp(os.path.join(ROOT, "examples", "multidimensional_scaling.cpp"), "example_multidimensional_scaling")
    r = subprocess.run([ex], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "Embedding dimension: 2" in r.stdout, r.stdout + r.stderr
    ex = build_cpp(os.path.join(ROOT, "examples", "principal_component_analysis.cpp"), "example_principal_component_analysis")
    r = subprocess.run([ex], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "Data mean: 0.5 50 500" in r.stdout, r.stdout + r.stderr
