"""The yardstick of the multidimensional-scaling and principal-component entries (rules M1-M5 and P1-P5 of c_api.h): a
numpy restatement.  The reference is not compiled (it needs Eigen and Spectra), so -- as for the spectral embedding -- the eigenpairs come from
dense f64 numpy.linalg.eigh of -1/2 J Dhat J built in f64 from the same f32-valued Dhat, and every other rule is transcribed from the
reference's lines:
    M1  squared (utilities/multidimensional_scaling.hpp:54-58: array().square() in ScalarT)
    M2  centred
    M3  sizes (:106-118, :40-42)
    M4  criterion (3rd_party/Spectra/HermEigsBase.h:152-167 with the float literal of :44), wanted (LargestMagn, :65-66)
    M5  clamp (:70-73), embedding_dim (estimateEmbeddingDimensionEigengap, :10-31), the sign rule
    P1-P5  pca_moments (core/covariance.hpp:64-76 with the entry's f64 sums), pca_eigen (core/principal_component_analysis.hpp:76-84), project,
           reconstruct (:46-68)
solve() is a numpy model of the device solver (locked, Chebyshev-filtered subspace iteration with an adaptive degree): it shows on the CPU that
every input of the GPU tests can be solved to rule M4, and that the one documented case cannot.  INPUTS names those inputs."""
import numpy as np

F32, F64 = np.float32, np.float64
FLT_EPS = float(np.finfo(F32).eps)
EPS23 = float(F32(FLT_EPS) ** (F32(2.0) / F32(3.0)))      # Spectra's eps23 for float
TOL = float(F32(1e-7))                                      # multidimensional_scaling.hpp:44


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def sqdist(P):
    """f32 matrix of squared distances of f64 points (computed in f64, rounded once; exactly symmetric, zero diagonal)"""
    P = np.asarray(P, F64)
    g = P @ P.T
    d = np.diag(g)[:, None] + np.diag(g)[None, :] - 2.0 * g
    d = 0.5 * (d + d.T)
    np.fill_diagonal(d, 0.0)
    return np.maximum(d, 0.0).astype(F32)


def circle(n=1000):
    """examples/multidimensional_scaling.cpp:11-29: the wobbling circle, squared distances in f32 as the example forms them"""
    i = np.arange(n, dtype=F32)
    two_pi = F32(2.0) * F32(np.pi)
    P = np.stack([np.cos(two_pi * i / F32(n)), np.sin(two_pi * i / F32(n)), F32(0.1) * np.sin(F32(10.0) * two_pi * i / F32(n))], 1).astype(F32)
    d = (P[:, None, :] - P[None, :, :]).astype(F32)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(F32) + d[..., 2] * d[..., 2]).astype(F32), P


def gauss5(n, seed=3):
    P = np.random.default_rng(seed + n).standard_normal((n, 5)) * np.array([5.0, 3.0, 2.0, 1.0, 0.5])
    return sqdist(P), P


def gauss40_iso(n=400, seed=7):
    P = np.random.default_rng(seed).standard_normal((n, 40))
    return sqdist(P), P


def gauss40_decay(n=513, seed=8):
    P = np.random.default_rng(seed).standard_normal((n, 40)) * (0.85 ** np.arange(40))
    return sqdist(P), P


def wavy_sheet(n=2049, seed=9):
    rng = np.random.default_rng(seed)
    u, v = rng.uniform(-2.0, 2.0, n), rng.uniform(-1.0, 1.0, n)
    P = np.stack([u, v, 0.3 * np.sin(2.0 * u) * np.cos(3.0 * v)], 1)
    return sqdist(P), P


def ring_geodesics(n=257):
    """squared geodesic distances on a ring of n points: not Euclidean -- the spectrum has degenerate pairs and negative values"""
    i = np.arange(n)
    k = np.abs(i[:, None] - i[None, :])
    g = np.minimum(k, n - k) * (2.0 * np.pi / n)
    return (g * g).astype(F32), None


def negative_dominant(n=65, seed=12):
    """a Euclidean cloud plus a rank-one term whose NEGATIVE eigenvalue dominates B"""
    P = np.random.default_rng(seed).standard_normal((n, 3)) * np.array([2.0, 1.0, 0.5])
    w = np.random.default_rng(seed + 1).standard_normal(n)
    d = sqdist(P).astype(F64) + 40.0 * np.outer(w, w)
    np.fill_diagonal(d, 0.0)
    return (0.5 * (d + d.T)).astype(F32), None


def simplex(n=64):
    d = np.ones((n, n), F32)
    np.fill_diagonal(d, 0.0)
    return d, None


def cloud3(n=300, seed=21):
    """a 3-D cloud with a simple spectrum: the MDS / PCA cross-check"""
    P = (np.random.default_rng(seed).standard_normal((n, 3)) * np.array([3.0, 1.5, 0.6])).astype(F32)
    return sqdist(P), P


# name -> (maker, [(max_dim, estimate_dim), ...]); every request is solved by solve() on the CPU (tests/test_mds_refs_cpu.py)
INPUTS = {
    "circle": (circle, [(2, False), (3, False)]),
    "gauss5_6": (lambda: gauss5(6), [(4, False)]), "gauss5_63": (lambda: gauss5(63), [(4, False)]), "gauss5_64": (lambda: gauss5(64), [(4, False)]),
    "gauss5_65": (lambda: gauss5(65), [(4, False)]), "gauss5_257": (lambda: gauss5(257), [(4, False)]),
    "gauss5_3": (lambda: gauss5(3), [(2, False)]), "gauss5_5": (lambda: gauss5(5), [(2, False)]),
    "gauss40_iso": (gauss40_iso, [(3, False), (3, True)]),
    "gauss40_decay": (gauss40_decay, [(16, False), (16, True)]),
    "wavy_sheet": (wavy_sheet, [(3, False)]),
    "ring": (ring_geodesics, [(2, False), (2, True), (3, False)]),
    "negative": (negative_dominant, [(3, False)]),
    "simplex": (simplex, [(2, False)]),
    "cloud3": (cloud3, [(3, False)]),
    # sizes around the kernel's edges: the 128-row chunk, the 64-row tile inside it, the 256- and 1024-column blocks
    "edge_127": (lambda: gauss5(127), [(2, False)]), "edge_128": (lambda: gauss5(128), [(2, False)]), "edge_129": (lambda: gauss5(129), [(2, False)]),
    "edge_255": (lambda: gauss5(255), [(2, False)]), "edge_256": (lambda: gauss5(256), [(2, False)]),
    "edge_1023": (lambda: gauss5(1023), [(2, False)]), "edge_1024": (lambda: gauss5(1024), [(2, False)]), "edge_1025": (lambda: gauss5(1025), [(2, False)]),
    "edge_1028": (lambda: gauss5(1028), [(2, False)]),
}
_cache = {}


def matrix(name):
    if name not in _cache:
        _cache[name] = INPUTS[name][0]()
    return _cache[name]


# ---- M1, M2 -----------------------------------------------------------------------------------------------------------------------
def squared(D, distances_are_squared=True):
    D = np.ascontiguousarray(D, F32)
    return D if distances_are_squared else (D * D).astype(F32)


def centred(Dhat):
    """B = -1/2 J Dhat J in f64"""
    A = np.asarray(Dhat, F64)
    r = A.mean(0)
    return -0.5 * (A - r[None, :] - A.mean(1)[:, None] + r.mean())


_eigh = {}


def spectrum(name, distances_are_squared=True):
    """dense f64 eigenpairs of B by descending magnitude -> (lam, Q, ||B||_2)"""
    if name not in _eigh:
        lam, Q = np.linalg.eigh(centred(matrix(name)[0]))
        order = np.argsort(-np.abs(lam), kind="stable")
        _eigh[name] = (lam[order], Q[:, order], float(np.abs(lam).max()))
    return _eigh[name]


# ---- M3 -----------------------------------------------------------------------------------------------------------------------------
def sizes(n, max_dim, estimate_dim):
    """:106-118 and :40-42 -> (dim, estimate, nev)"""
    if not (max_dim > 0 and max_dim < n):
        max_dim, estimate_dim = 2, False
    return max_dim, bool(estimate_dim), (min(max_dim + 1, n - 1) if estimate_dim else max_dim)


# ---- M4 -----------------------------------------------------------------------------------------------------------------------------
def criterion(theta):
    return TOL * np.maximum(EPS23, np.abs(np.asarray(theta, F64)))


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def eigenvalue_bound(lam_ref, n, norm):
    """|theta - lambda_ref| <=: Weyl on the accepted residual, the rounding to f32, the yardstick's own error"""
    lam_ref = np.asarray(lam_ref, F64)
    return 1e-7 * np.maximum(FLT_EPS ** (2.0 / 3.0), np.abs(lam_ref)) + 0.5 * ulp32(lam_ref) + n * np.finfo(F64).eps * norm


# ---- M5 -----------------------------------------------------------------------------------------------------------------------------
def clamp(theta):
    ev = np.asarray(theta, F64).astype(F32)
    ev[ev < 0] = F32(0.0)
    return ev


def embedding_dim(ev, max_dim):
    """estimateEmbeddingDimensionEigengap, utilities/multidimensional_scaling.hpp:10-31, line by line in f32"""
    ev = np.asarray(ev, F32)
    min_val, max_val, max_diff, max_ind = F32(np.inf), F32(-np.inf), F32(-np.inf), 0
    for i in range(len(ev) - 1):
        diff = F32(ev[i] - ev[i + 1])
        if diff > max_diff:
            max_diff, max_ind = diff, i
        if ev[i] < min_val:
            min_val = ev[i]
        if ev[i] > max_val:
            max_val = ev[i]
    if ev[-1] < min_val:
        min_val = ev[-1]
    if ev[-1] > max_val:
        max_val = ev[-1]
    if F32(max_val - min_val) < F32(FLT_EPS):
        return max_dim
    return max_ind + 1


def signed(Q):
    """the sign rule: the largest-magnitude component of each column positive, the lowest index among equals"""
    Q = np.asarray(Q, F64)
    pick = np.argmax(np.abs(Q), axis=0)
    return Q * np.where(Q[pick, np.arange(Q.shape[1])] < 0, -1.0, 1.0)[None, :]


def embedding(ev, Q, dim):
    """sqrtf(ev[c]) * (float)(signed x)"""
    return (np.sqrt(np.asarray(ev, F32)[:dim])[None, :] * signed(Q[:, :dim]).astype(F32)).astype(F32)


# ---- the solver's model ---------------------------------------------------------------------------------------------------------------
def start_block(n, b):
    """the device's start block: splitmix64's finaliser of (row * 64 + column + 1), uniform in [-1, 1)"""
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(64) + np.arange(b, dtype=np.uint64)[None, :] + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(F64) * (1.0 / 4503599627370496.0) - 1.0


def filter_plan(a0, least, lowest_wanted, top_locked, max_degree):
    """csrc/mds_host.hpp: mds_filter_plan -> (e, degree)"""
    e = least
    if not (e < a0 * (1.0 - 1e-3)) or not (e > 0.0):
        e = 0.5 * a0
    lo = max(lowest_wanted, e)
    at_a0 = np.arccosh(a0 / e)
    spread = at_a0 - np.arccosh(lo / e)
    above = np.arccosh(top_locked / e) - at_a0 if top_locked > a0 else 0.0
    m = max_degree
    if spread > 0.0 and m * spread > np.log(1e6):
        m = int(np.floor(np.log(1e6) / spread))
    if above > 0.0 and m * above > np.log(1e10):
        m = int(np.floor(np.log(1e10) / above))
    return e, max(m, 1)


def _cholqr2(X, first):
    """SubspaceOps::orthonormalise: CholQR2 of the columns from `first` on, scaled to unit length first; a Gram matrix that is not positive
    definite (the filter drowned an unwanted column) is shifted, and a shifted pass is followed by more passes (4 at the most)"""
    passes, p = 2, 0
    while p < passes:
        A = X[:, first:]
        d = np.sqrt(np.einsum("ij,ij->j", A, A))
        d[~((d > 0) & np.isfinite(d))] = 1.0
        G = (A.T @ A) / np.outer(d, d)
        G = 0.5 * (G + G.T)
        shift = 0.0
        for attempt in range(9):
            try:
                R = np.linalg.cholesky(G).T
                break
            except np.linalg.LinAlgError:
                if attempt == 8:
                    raise
                add = 1e-13 * len(d) if shift == 0.0 else shift * 99.0
                G = G + add * np.eye(len(d))
                shift += add
                passes = max(passes, min(p + 3, 4))
        X[:, first:] = (A / d[None, :]) @ np.linalg.inv(R)
        p += 1
    return X


def solve(D, max_dim=2, estimate_dim=False, distances_are_squared=True, max_outer=1000, degree=24, guard=3):
    """-> dict(dim, nev, n_converged, outer, products, theta (magnitude order), X, residual)"""
    B = centred(squared(D, distances_are_squared))
    n = len(B)
    dim, estimate, nev = sizes(n, max_dim, estimate_dim)
    b = min(nev + max(guard, nev // 2), n)
    X = _cholqr2(start_block(n, b), 0)
    AX = np.zeros_like(X)
    theta, locked, outer, products = np.zeros(b), 0, 0, 0
    while True:
        outer += 1
        AX[:, locked:] = B @ X[:, locked:]
        products += 1
        G = X[:, locked:].T @ AX[:, locked:]
        w, S = np.linalg.eigh(0.5 * (G + G.T))
        order = np.argsort(-np.abs(w), kind="stable")
        X[:, locked:], AX[:, locked:], theta[locked:] = X[:, locked:] @ S[:, order], AX[:, locked:] @ S[:, order], w[order]
        res = np.linalg.norm(AX - X * theta[None, :], axis=0)
        while locked < nev and res[locked] < criterion(theta[locked]):
            locked += 1
        if locked == nev or outer >= max_outer:
            break
        a0 = abs(theta[locked])
        e, m = filter_plan(a0, abs(theta[b - 1]), abs(theta[nev - 1]), abs(theta[0]) if locked else 0.0, degree)
        sigma1 = sigma = e / a0
        Yp, Yc = X[:, locked:], (sigma1 / e) * (B @ X[:, locked:])
        for _ in range(2, m + 1):
            sigma2 = 1.0 / (2.0 / sigma1 - sigma)
            Yp, Yc = Yc, (2.0 * sigma2 / e) * (B @ Yc) - sigma * sigma2 * Yp
            sigma = sigma2
        products += m
        X[:, locked:] = Yc
        for _ in range(2):
            X[:, locked:] -= X[:, :locked] @ (X[:, :locked].T @ X[:, locked:])
        X = _cholqr2(X, locked)
    order = np.argsort(-np.abs(theta[:nev]), kind="stable")
    return dict(dim=dim, estimate=estimate, nev=nev, n_converged=locked, outer=outer, products=products, theta=theta[:nev][order], X=X[:, :nev][:, order],
                residual=float(res[:nev].max()))


# ---- P1-P5 ----------------------------------------------------------------------------------------------------------------------------
def two_stage(n):
    nb = min(256, max((n + 63) // 64, 1))
    return nb, (n + nb - 1) // nb


def _ordered_sum(terms):
    """f64 sum over axis 0 in the entry's order: chunks of two_stage(count) consecutive rows, ascending inside a chunk, the chunks' sums added
    in ascending order (np.cumsum adds sequentially)"""
    count = len(terms)
    nb, rows = two_stage(count)
    total = np.zeros(terms.shape[1:], F64)
    for lo in range(0, count, rows):
        total = total + np.cumsum(terms[lo:lo + rows], axis=0)[-1]
    return total


def pca_moments(x, subset=None):
    """core/covariance.hpp:31-180 with the entry's arithmetic: P1, P2, P3 -> (mean f32, cov f32, valid)"""
    x = np.ascontiguousarray(x, F32)
    pts = x if subset is None else x[np.asarray(subset, np.int64)]
    count, D = pts.shape
    if count < 2:
        return np.full(D, np.nan, F32), np.full((D, D), np.nan, F32), False
    mean = (_ordered_sum(pts.astype(F64)) / count).astype(F32)
    tmp = (pts - mean[None, :]).astype(F32).astype(F64)
    cov = (_ordered_sum(tmp[:, :, None] * tmp[:, None, :]) / (count - 1)).astype(F32)
    return mean, cov, True


def pca_eigen(cov):
    """principal_component_analysis.hpp:76-84 -> (eigenvalues f64 descending, eigenvectors f64 as ROWS); columns 0 .. D-2 by the sign rule,
    the last one makes the determinant positive"""
    lam, Q = np.linalg.eigh(np.asarray(cov, F32).astype(F64))
    lam, Q = lam[::-1], Q[:, ::-1].copy()
    D = len(lam)
    if D > 1:
        Q[:, :D - 1] = signed(Q[:, :D - 1])
    if np.linalg.det(Q) < 0:
        Q[:, D - 1] = -Q[:, D - 1]
    return lam, Q.T.copy()


def project(x, mean, vectors, target_dim):
    """:46-49: x - mean in f32; products (exact in f64) and their sum over ascending coordinates in f64, rounded once"""
    t = (np.asarray(x, F32) - np.asarray(mean, F32)[None, :]).astype(F32).astype(F64)
    V = np.asarray(vectors, F32).astype(F64)
    out = np.zeros((len(t), target_dim), F64)
    for k in range(t.shape[1]):
        out = out + t[:, k:k + 1] * V[None, :target_dim, k]
    return out.astype(F32)


def reconstruct(y, mean, vectors):
    """:59-62: the first y.shape[1] vectors; the f64 sum over ascending vectors, plus the mean, rounded once"""
    y = np.asarray(y, F32).astype(F64)
    V = np.asarray(vectors, F32).astype(F64)
    out = np.zeros((len(y), V.shape[1]), F64)
    for t in range(y.shape[1]):
        out = out + y[:, t:t + 1] * V[None, t, :]
    return (out + np.asarray(mean, F32).astype(F64)[None, :]).astype(F32)
