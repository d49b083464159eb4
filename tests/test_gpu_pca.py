"""GPU: cilhip_pca_fit / cilhip_pca_project / cilhip_pca_reconstruct and the Python mirror against tests/_mds_refs.py -- DESIGN.md section 19,
rules P1-P5 of c_api.h -- and the identity that ties the two halves of that section together: on Euclidean input classical MDS and PCA give
the same coordinates.  Every bound is derived where it is used; each test prints its figures before it asserts."""
import numpy as np
import pytest

import _mds_refs as R
from cilantro_amd import capi

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EPS32, EPS64 = float(np.finfo(F32).eps), float(np.finfo(F64).eps)
DIMS = [1, 2, 3, 7, 16]
SIZES = [1, 2, 3, 255, 256, 257, 65537]      # 65 537: past the 256 x 256 shape of the two-stage sum
_cache = {}


def data(n, D):
    """off-origin: mean 1e3, spread 1 along the first axis and less along the others -- a one-pass formula loses every digit here"""
    if (n, D) not in _cache:
        rng = np.random.default_rng(100 * D + n % 97)
        _cache[(n, D)] = (1e3 + rng.standard_normal((n, D)) * (0.8 ** np.arange(D))).astype(F32)
    return _cache[(n, D)]


def fit(x, subset=None):
    from cilantro_amd.principal_component_analysis import PrincipalComponentAnalysis

    return PrincipalComponentAnalysis(x, subset)


def _check_eigen(cov, values, vectors):
    """vectors: the reference's matrix (vector c is column c)"""
    D = len(values)
    C64 = cov.astype(F64)
    lam = np.linalg.eigvalsh(C64)[::-1]
    norm = float(np.abs(lam).max())
    # cyclic Jacobi is accurate to a few D eps64 ||C||; the outputs are rounded to f32
    tiny = 64.0 * D * EPS64 * norm
    err = np.abs(values.astype(F64) - lam)
    print("eigenvalues", values, "error", err.max(), "bound", 0.5 * R.ulp32(lam).max() + tiny)
    assert (err <= 0.5 * R.ulp32(lam) + tiny).all() and (np.diff(values) <= 0).all()
    V = vectors.astype(F64)
    # entries rounded to f32: ||dV||_F <= eps32 / 2 sqrt(D)
    assert np.linalg.norm(V.T @ V - np.eye(D), 2) <= EPS32 * np.sqrt(D) + tiny / max(norm, 1e-300)
    res = np.linalg.norm(C64 @ V - V * values.astype(F64)[None, :], axis=0)
    print("residuals", res.max(), "bound", norm * 2.0 * EPS32 + tiny)
    assert (res <= norm * 2.0 * EPS32 + tiny).all()
    assert np.linalg.det(V) > 0
    for c in range(D - 1):
        assert vectors[:, c].max() == np.abs(vectors[:, c]).max(), "sign rule"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("D", DIMS)
def test_fit(D, n):
    x = data(n, D)
    p = fit(x)
    mean, cov, valid = R.pca_moments(x)
    assert p.isValid() == valid == (n >= 2)
    if not valid:      # P3
        assert np.isnan(p.getDataMean()).all() and np.isnan(p.getDataCovariance()).all() and np.isnan(p.getEigenValues()).all() and np.isnan(p.getEigenVectors()).all()
        return
    print(f"D {D} n {n}: mean {p.getDataMean()[:3]} cov[0, 0] {p.getDataCovariance()[0, 0]}")
    # the restatement pins the order of the sums: bit for bit
    assert p.getDataMean().tobytes() == mean.tobytes()
    assert p.getDataCovariance().tobytes() == cov.tobytes()
    _check_eigen(cov, p.getEigenValues(), p.getEigenVectors())


def test_simple_spectrum_gives_the_reference_vectors():
    x = data(257, 3)
    p = fit(x)
    lam, Q = R.pca_eigen(p.getDataCovariance())
    gap = np.min(np.abs(np.diff(lam)))
    # Davis-Kahan with Jacobi's accuracy as the residual, and the rounding of the entries to f32
    bound = np.sqrt(2.0) * 64.0 * 3 * EPS64 * lam[0] / gap + EPS32
    err = np.abs(p.getEigenVectors().T.astype(F64) - Q).max()
    print("vectors: error", err, "bound", bound, "gap", gap)
    assert err <= bound


def test_subset_and_an_index_out_of_range():
    x = data(257, 7)
    subset = np.random.default_rng(4).permutation(257)[:100].astype(np.uint32)
    p = fit(x, subset)
    mean, cov, _ = R.pca_moments(x, subset)
    assert p.getDataMean().tobytes() == mean.tobytes() and p.getDataCovariance().tobytes() == cov.tobytes()
    assert not fit(x, subset[:1]).isValid()
    import torch

    q = fit(torch.from_numpy(x).cuda(), torch.from_numpy(subset.astype(np.int64)).cuda())
    assert q.getDataCovariance().tobytes() == cov.tobytes()
    bad = subset.copy()
    bad[57] = 257
    with pytest.raises(capi.CilhipError) as e:
        fit(x, bad)
    print(e.value)
    assert e.value.code == capi.ERR_INVALID and "subset" in str(e.value)


def test_the_box_of_the_example():
    """examples/principal_component_analysis.cpp: the corners of a 1 x 100 x 1000 box"""
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 100, 0], [0, 0, 1000], [0, 100, 1000], [1, 0, 1000], [1, 100, 0], [1, 100, 1000]], F32)
    p = fit(pts)
    print(p.getDataMean(), p.getEigenValues(), p.getEigenVectors())
    assert (p.getDataMean() == np.array([0.5, 50.0, 500.0], F32)).all()
    assert np.allclose(p.getEigenValues(), np.array([1000.0 ** 2, 100.0 ** 2, 1.0]) * 2.0 / 7.0, rtol=2 * EPS32, atol=0)
    V = p.getEigenVectors()
    assert (np.abs(V) == np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], F32)).all()      # axes +-e_z, +-e_y, +-e_x
    assert V[2, 0] == 1 and V[1, 1] == 1 and np.linalg.det(V.astype(F64)) > 0


PCA_TRIP = 2048 * 256      # k_pca_project / k_pca_reconstruct: sp_grid(m, 2048) blocks of SP_THREADS = 256 lanes, a row per lane and trip


@pytest.mark.parametrize("D,n", [(1, 3), (2, 257), (3, 65537), (7, 256), (16, 255), (3, 600001)])      # 600 001: 75 713 rows in a second trip
def test_project_and_reconstruct(D, n):
    import torch

    x = data(n, D)
    p = fit(x)
    mean, V = p.getDataMean(), p.getEigenVectors().T.copy()      # rows
    for t in sorted({1, (D + 1) // 2, D}):
        y = p.project(x, t)
        assert y.tobytes() == R.project(x, mean, V, t).tobytes()
        assert p.reconstruct(y).tobytes() == R.reconstruct(y, mean, V).tobytes()
    yd = p.project(torch.from_numpy(x).cuda(), D)
    assert yd.is_cuda and yd.cpu().numpy().tobytes() == y.tobytes()
    back = p.reconstruct(y)
    # V^T V = I up to the f32 rounding of V's entries (eps32 sqrt(D) in norm), the projection is rounded once (eps32 / 2 in norm), the
    # difference x - mean and the result are each rounded to f32 at the size of x
    span = float(np.linalg.norm(x.astype(F64) - mean.astype(F64), axis=1).max())
    bound = span * EPS32 * (np.sqrt(D) + 1.0) + EPS32 * float(np.abs(x).max())
    err = float(np.abs(back.astype(F64) - x.astype(F64)).max())
    print(f"D {D} n {n}: round trip error {err:.3e} bound {bound:.3e}")
    assert err <= bound
    if n > PCA_TRIP:      # a row of the last trip is as accurate as one of the first: the same bound on its own rows, the same bits as the restatement
        last = float(np.abs(back[PCA_TRIP:].astype(F64) - x[PCA_TRIP:].astype(F64)).max())
        print(f"rows {PCA_TRIP} .. {n - 1}: round trip error {last:.3e}")
        assert last <= bound and y[PCA_TRIP:].tobytes() == R.project(x[PCA_TRIP:], mean, V, D).tobytes()
        assert back[PCA_TRIP:].tobytes() == R.reconstruct(y[PCA_TRIP:], mean, V).tobytes() and np.isfinite(back[PCA_TRIP:]).all()
    with pytest.raises(capi.CilhipError):
        p.project(x, D + 1)


def test_nothing_stays_allocated():
    import ctypes as C

    def live():
        out = (C.c_ulonglong * 2)()
        assert capi.load().cilhip_debug_live_allocations(out) == capi.OK
        return out[0], out[1]

    before = live()
    x = data(257, 7)
    p = fit(x, np.arange(100, dtype=np.uint32))
    p.reconstruct(p.project(x, 3))
    with pytest.raises(capi.CilhipError):
        fit(x, np.array([0, 1, 999], np.uint32))
    assert live() == before


def test_mds_of_the_distances_is_pca_of_the_points():
    """MultidimensionalScaling3f of the squared distances = PrincipalComponentAnalysis3f::project of the points, up to the sign per axis, and
    lambda_mds = (n - 1) lambda_pca.  The bound is the sum of the two sides' own: MDS sees B perturbed by the f32 rounding of the distances
    (||dB|| <= ||dD||_F <= eps32 / 2 ||D||_F) and stops at the accepted residual; PCA sees a covariance perturbed by the f32 rounding of
    x - mean and of its own entries (2 eps32 ||C||_F) and projects with f32 vectors; Davis-Kahan turns both into angles."""
    from cilantro_amd.multidimensional_scaling import MultidimensionalScaling3f

    D, P = R.matrix("cloud3")
    n = len(P)
    mds = MultidimensionalScaling3f(D)
    p = fit(P)
    proj = p.project(P, 3).astype(F64)
    Y = mds.getEmbeddedPoints().astype(F64)
    lam_b = R.spectrum("cloud3")[0]
    norm_b = float(np.abs(lam_b).max())
    lam_c = p.getEigenValues().astype(F64)
    dB = 0.5 * EPS32 * float(np.linalg.norm(D.astype(F64)))
    dC = 2.0 * EPS32 * float(np.linalg.norm(p.getDataCovariance().astype(F64)))
    centred = P.astype(F64) - P.astype(F64).mean(0)
    for c in range(3):
        gap_b = float(np.min(np.abs(np.delete(lam_b, c) - lam_b[c])))
        gap_c = float(np.min(np.abs(np.delete(lam_c, c) - lam_c[c])))
        root = np.sqrt(lam_b[c])
        b_mds = root * (np.sqrt(2.0) * (float(R.criterion(lam_b[c])) + dB + n * EPS64 * norm_b) / gap_b + 4.0 * EPS32)
        b_pca = np.linalg.norm(centred, 2) * (np.sqrt(2.0) * dC / gap_c + EPS32) + 2.0 * EPS32 * root + 0.5 * EPS32 * float(np.abs(p.getDataMean()).max()) * np.sqrt(n)
        y = Y[:, c] if Y[:, c] @ proj[:, c] >= 0 else -Y[:, c]
        err = float(np.linalg.norm(y - proj[:, c]))
        print(f"axis {c}: ||mds - pca|| {err:.3e} bound {b_mds + b_pca:.3e} ({b_mds:.3e} + {b_pca:.3e})")
        assert err <= b_mds + b_pca
        ev_m, ev_p = float(mds.getComputedEigenValues()[c]), (n - 1) * lam_c[c]
        b_ev = float(R.eigenvalue_bound(lam_b[c], n, norm_b)) + dB + (n - 1) * (dC + 0.5 * float(R.ulp32(lam_c[c])))
        print(f"axis {c}: eigenvalue {ev_m:.8g} against (n - 1) * {lam_c[c]:.8g} = {ev_p:.8g}, bound {b_ev:.3e}")
        assert abs(ev_m - ev_p) <= b_ev
