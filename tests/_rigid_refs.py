"""The yardstick of the rigid-fit tests (numpy, f64, no GPU): the closed-form point-to-point fit of
registration/transform_estimation.hpp:11-48 judged by the property it is defined by -- the returned rigid motion minimises
sum |R s + t - d|^2 over the PROPER rotations -- and not by element-wise parity, which is unpinned wherever the cross-covariance is
rank-deficient (the rotation is then not unique).

    optimum(dst, src) -> the optimal cost C*, the cost scale and one optimal (R, t)
    cost(T, dst, src) -> sum |R s + t - d|^2 of a returned f32 4x4, in f64
    bound(dst, src, T) -> how far cost may lie above C* (derived where the function is)
    check(T, dst, src) -> finite, bottom row 0 0 0 1, orthogonal to 4 u, det > 0, cost - C* <= bound
    cases(frame) -> the table of degenerate, mirrored and generic pair sets, in one of FRAMES
"""
import numpy as np

from cilantro_amd import synthetic as syn

F32, F64 = np.float32, np.float64
U32 = 2.0 ** -24                      # unit round-off of f32
EPS64 = 2.0 ** -52

BASE_R = syn.rot_xyz(0.25, -0.4, 0.1)
BASE_T = np.array([0.2, 0.1, -0.3])
MIRROR_Z = np.diag([1.0, 1.0, -1.0])

FRAMES = (("as is", 1.0, (0.0, 0.0, 0.0)), ("at (1e3, -250, 37)", 1.0, (1e3, -250.0, 37.0)), ("x 2^12", 2.0 ** 12, (0.0, 0.0, 0.0)),
          ("x 2^-12", 2.0 ** -12, (0.0, 0.0, 0.0)))


def _centred(dst, src):
    d, s = np.asarray(dst, F64).reshape(-1, 3), np.asarray(src, F64).reshape(-1, 3)
    if len(d) == 0:
        return d, s, np.zeros(3), np.zeros(3)
    md, ms = d.mean(axis=0), s.mean(axis=0)
    return d - md, s - ms, md, ms


def optimum(dst, src, flip_col=2, flip=True):
    """-> (C*, scale, R, t).  H = dc^T sc = U S V^T; the best proper rotation is U diag(1, 1, sgn) V^T, sgn = sign det(U V^T), and
    C* = |dc|^2 + |sc|^2 - 2 (S0 + S1 + sgn S2).  R is that rotation formed as the reference forms it: the LAST column of U negated
    (transform_estimation.hpp:38-41).  flip_col / flip: the wrong variants of the negative controls."""
    dc, sc, md, ms = _centred(dst, src)
    if len(dc) == 0:
        return 0.0, 0.0, np.eye(3), np.zeros(3)
    U, S, Vt = np.linalg.svd(dc.T @ sc)
    sgn = 1.0 if np.linalg.det(U @ Vt) >= 0.0 else -1.0
    scale = float((dc * dc).sum() + (sc * sc).sum())
    c_opt = scale - 2.0 * float(S[0] + S[1] + sgn * S[2])
    if flip and sgn < 0.0:
        U = U.copy()
        U[:, flip_col] = -U[:, flip_col]
    R = U @ Vt
    return c_opt, scale, R, md - R @ ms


def pack(R, t):
    """(R, t) -> the f32 4x4 an estimator returns"""
    T = np.eye(4, dtype=F32)
    T[:3, :3] = np.asarray(R, F64).astype(F32)
    T[:3, 3] = np.asarray(t, F64).astype(F32)
    return T


def cost(T, dst, src):
    T = np.asarray(T, F64).reshape(4, 4)
    d, s = np.asarray(dst, F64).reshape(-1, 3), np.asarray(src, F64).reshape(-1, 3)
    e = s @ T[:3, :3].T + T[:3, 3] - d
    return float((e * e).sum())


def bound(dst, src, T):
    """The allowed excess of cost(T) over C*, from two terms and nothing else.

    The estimator forms sigma = sum d s^T / n - mean_d mean_s^T from raw f64 moments, takes (R, t) from it in f64 and returns the
    twelve numbers rounded to f32.

    (2) Raw-moment cancellation.  Each entry of sum d s^T is a sum of n products of f32 values (exact in f64) added in f64, the
        two means are sums of n terms, and the division, the product of the means and the subtraction round once each: the entry
        of sigma carries an error of at most (n + 4) eps64 max|d| max|s|, so |E|_F <= 3 (n + 4) eps64 max|d| max|s| over the nine
        entries.  With H = n sigma the cost of a rotation is scale - 2 tr(R^T H); the rotation R' that is optimal for H + n E
        loses at most tr(R*^T H) - tr(R'^T H) <= 2 n max_R |tr(R^T E)| <= 2 sqrt(3) n |E|_F of the trace (|R|_F = sqrt(3)),
        i.e. its cost is at most C* + 4 sqrt(3) n |E|_F.  (t = mean_d - R mean_s is optimal for whatever R is.)
    (1) Output rounding.  With u = 2^-24 every entry of R moves by at most u |R_jk| and t by u |t| per component, so residual
        i moves by at most delta_i = u (sqrt(3) |s_i| + |t|): row j of dR times s_i is at most u |R_j| |s_i| = u |s_i|, three
        rows.  (|t| is read off the rounded output: |t_f64| <= |t_f32| / (1 - u).)  By the triangle inequality in R^(3n),
        sqrt(cost) <= sqrt(cost before rounding) + sqrt(sum delta_i^2).

    Together: cost <= (sqrt(C* + 4 sqrt(3) n |E|_F) + sqrt(sum delta_i^2))^2, and the bound is that minus C*."""
    d, s = np.asarray(dst, F64).reshape(-1, 3), np.asarray(src, F64).reshape(-1, 3)
    n = len(d)
    if n == 0:
        return 0.0
    c_opt = max(optimum(d, s)[0], 0.0)
    e_f = 3.0 * (n + 4) * EPS64 * float(np.abs(d).max()) * float(np.abs(s).max())
    t2 = 4.0 * np.sqrt(3.0) * n * e_f
    tn = float(np.linalg.norm(np.asarray(T, F64).reshape(4, 4)[:3, 3])) / (1.0 - U32)
    delta = U32 * (np.sqrt(3.0) * np.linalg.norm(s, axis=1) + tn)
    return float((np.sqrt(c_opt + t2) + np.sqrt(float((delta * delta).sum()))) ** 2 - c_opt)


def figures(T, dst, src):
    """-> dict(excess, bound, scale, ortho, det) of a returned transform"""
    T = np.asarray(T)
    R = T.astype(F64).reshape(4, 4)[:3, :3]
    c_opt, scale, _, _ = optimum(dst, src)
    finite = bool(np.isfinite(T).all())
    return {"excess": cost(T, dst, src) - c_opt if finite else float("nan"), "bound": bound(dst, src, T) if finite else float("nan"), "scale": scale,
            "ortho": float(np.abs(R.T @ R - np.eye(3)).max()) if finite else float("nan"), "det": float(np.linalg.det(R)) if finite else float("nan")}


def check(T, dst, src, tag=""):
    """asserts what a rigid fit of the pairs (dst_i, src_i) must be; prints excess and bound first -> the figures"""
    T = np.asarray(T)
    f = figures(T, dst, src)
    print(f"{tag}: n {len(np.asarray(dst).reshape(-1, 3))} excess {f['excess']:.3e} bound {f['bound']:.3e} scale {f['scale']:.3e} "
          f"|R^T R - I| {f['ortho']:.2e} det {f['det']:.6f}")
    assert T.shape == (4, 4) and T.dtype == F32, (tag, T.shape, T.dtype)
    assert np.isfinite(T).all(), (tag, "not finite", T.tolist())
    assert np.array_equal(T[3], np.array([0, 0, 0, 1], F32)), (tag, "bottom row", T[3].tolist())
    assert f["ortho"] <= 4.0 * U32, (tag, "not orthogonal", f["ortho"])
    assert f["det"] > 0.0, (tag, "a reflection", f["det"])
    assert f["excess"] <= f["bound"], (tag, "not optimal", f["excess"], f["bound"])
    return f


def passes(T, dst, src):
    """check() as a predicate, for the negative controls"""
    import contextlib
    import io

    try:
        with contextlib.redirect_stdout(io.StringIO()):
            check(T, dst, src)
    except AssertionError:
        return False
    return True


def rotated_by(T, angle):
    """T with its rotation block turned by `angle` about (1, 1, 1) / sqrt(3); the translation stays"""
    a = np.ones(3) / np.sqrt(3.0)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rd = np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)
    return pack(Rd @ np.asarray(T, F64)[:3, :3], np.asarray(T, F64)[:3, 3])


# ---- the case table -----------------------------------------------------------------------------------------------------------
def _base(src, R=BASE_R):
    return src @ R.T + BASE_T


def _table64():
    """(name, dst, src) in f64, before the frame"""
    out = []
    g = np.random.default_rng(101).random((3, 3))
    out.append(("3 generic", _base(g), g))
    out.append(("1 pair", _base(g[:1]), g[:1]))
    out.append(("2 pairs", _base(g[:2]), g[:2]))
    rep = g[[0, 0, 1]]
    out.append(("3 with a repeated point", _base(rep), rep))
    same = g[[0, 0, 0]]
    out.append(("3 identical", _base(same), same))
    line = g[0] + np.array([[0.0], [1.0], [2.5]]) * (g[1] - g[0])
    out.append(("3 collinear", _base(line), line))
    out.append(("3 mirrored in z", _base(g @ MIRROR_Z), g))
    p = np.random.default_rng(102).random((500, 3))
    out.append(("500 generic", _base(p), p))
    out.append(("500 mirrored in z", _base(p @ MIRROR_Z), p))
    flat = p.copy()
    flat[:, 2] = 0.5
    out.append(("500 coplanar", _base(flat), flat))
    ax = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    out.append(("500 under a rotation by pi", _base(p, 2.0 * np.outer(ax, ax) - np.eye(3)), p))
    out.append(("500 unrelated", np.random.default_rng(103).random((500, 3)), p))
    out.append(("500 mirrored, 1e-3 noise", _base(p @ MIRROR_Z) + np.random.default_rng(104).normal(0.0, 1e-3, (500, 3)), p))
    return out


MIRRORED_500 = ("500 mirrored in z", "500 mirrored, 1e-3 noise")
GENERIC_500 = ("500 generic", "500 under a rotation by pi")
THREE_PAIR = ("3 generic", "3 with a repeated point", "3 identical", "3 collinear", "3 mirrored in z")


def in_frame(x, scale, offset):
    """scaled and moved in f64, rounded once to f32"""
    return np.ascontiguousarray((np.asarray(x, F64) * scale + np.asarray(offset, F64)).astype(F32))


def cases(frame=0):
    """-> [(name, dst, src)], f32, in FRAMES[frame]"""
    _, scale, off = FRAMES[frame]
    return [(name, in_frame(d, scale, off), in_frame(s, scale, off)) for name, d, s in _table64()]


def family(kind, n, seed=0):
    """n pairs of the generic, the mirrored or the coplanar family (f32), for the size sweep"""
    p = np.random.default_rng(200 + seed).random((n, 3))
    if kind == "coplanar":
        p[:, 2] = 0.5
    d = _base(p @ MIRROR_Z) if kind == "mirrored" else _base(p)
    return in_frame(d, 1.0, 0.0), in_frame(p, 1.0, 0.0)
