"""numpy / scipy restatement of DESIGN.md section 17 (non-rigid ICP on a sparse warp field), the yardstick of tests/test_gpu_warp_field.py.

The reference's estimator (registration/warp_field_estimation.hpp:1388-1846) is restated the way it runs: a CSC Jacobian `At` (unknowns x
equations) with scipy.sparse, the explicit product `AtA = At At^T`, `Atb`, Eigen's Jacobi-preconditioned conjugate_gradient() from x0 = 0.
Every function takes a dtype: np.float32 is "the reference as it runs", np.float64 "the exact answer" (the control and regularisation
weights are DATA in both: the f32 values of the pinned exp, as the device forms them).  The reference's own binary cannot be the yardstick:
it needs Eigen, which the oracle build does not have.

Two forms of the assembly: `assemble` is vectorised over the correspondences (every element goes through the same operations in the same
order), `assemble_literal` is the reference's loop transcribed row by row; tests/test_warp_refs_cpu.py pins one against the other, and the
dense estimator's system (:369-716, `assemble_dense_literal`) against the sparse one with every source point its own control node.

Layouts: transforms are (n, 4, 4) arrays T[i][r, c]; tforms_vec is (6 n_ctrl,) = (a, b, c, tx, ty, tz) per node; lists are (n, k) uint32
index arrays padded with NONE and (n, k) float32 squared distances, as cilhip_knn3f writes them."""
import numpy as np
import scipy.sparse as sp

F = np.float32
NONE = 0xFFFFFFFF
UNITY, RBF = 0, 1


class Params:
    """cilhip_warp_params with the reference's values (icp_warp_field_combined_metric_sparse.hpp:67-70, warp_field_estimation.hpp:1411-1415)"""

    def __init__(self, w_p2p=0.0, w_p2pl=1.0, w_reg=1.0, huber_boundary=1e-4, max_gn_iter=10, gn_conv_tol=1e-5, max_cg_iter=1000, cg_conv_tol=1e-5):
        self.w_p2p, self.w_p2pl, self.w_reg, self.huber_boundary = F(w_p2p), F(w_p2pl), F(w_reg), F(huber_boundary)
        self.max_gn_iter, self.gn_conv_tol, self.max_cg_iter, self.cg_conv_tol = int(max_gn_iter), F(gn_conv_tol), int(max_cg_iter), F(cg_conv_tol)


# ---- lists and weights -----------------------------------------------------------------------------------------------------------
def d2_pinned(q, p):
    """(dx dx + dy dy) + dz dz in f32, every operation rounded once: (len(q), len(p))"""
    q, p = np.asarray(q, F), np.asarray(p, F)
    d = q[:, None, :] - p[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_lists(ref, query, k, max_sq=np.inf, chunk=4096):
    """brute-force k-NN lists in the layout of cilhip_knn3f: ascending distance, ties by lowest index, padded with NONE"""
    ref, query = np.asarray(ref, F), np.asarray(query, F)
    idx = np.full((len(query), k), NONE, np.uint32)
    d2 = np.zeros((len(query), k), F)
    for s in range(0, len(query), chunk):
        D = d2_pinned(query[s:s + chunk], ref)
        order = np.argsort(D, axis=1, kind="stable")[:, :k]
        dd = np.take_along_axis(D, order, axis=1)
        kk = order.shape[1]
        ok = dd < max_sq
        idx[s:s + chunk, :kk] = np.where(ok, order, NONE)
        d2[s:s + chunk, :kk] = np.where(ok, dd, 0)
    return idx, d2


def nearest(dst, q, max_sq):
    """the context's exact 1-NN: argmin of the pinned d2, lowest index on ties, kept when d2 < max_sq; NONE otherwise"""
    nn = np.empty(len(q), np.uint32)
    for s in range(0, len(q), 2048):
        D = d2_pinned(q[s:s + 2048], dst)
        j = np.argmin(D, axis=1)
        nn[s:s + 2048] = np.where(D[np.arange(len(j)), j] < max_sq, j, NONE)
    return nn


def eval_weights(kernel, sigma, d2):
    """eval(d2) in f32: 1 (Unity) or pinned_expf((-0.5f / (sigma sigma)) d2) (RBF on the squared distance)"""
    d2 = np.asarray(d2, F)
    if kernel == UNITY:
        return np.ones(d2.shape, F)
    from oracle import oracle as orc

    coeff = F(-0.5) / (F(sigma) * F(sigma))
    with np.errstate(all="ignore"):
        return orc.pinned_expf((coeff * d2).astype(F)).reshape(d2.shape).astype(F)


class Graph:
    """what cilhip_warp_field_create builds: weights, totals in list order (:1456-1465), arcs (:1736-1748)"""

    def __init__(self, n_ctrl, ctrl_idx, ctrl_d2, ctrl_kernel, ctrl_sigma, reg_idx, reg_d2, reg_kernel, reg_sigma):
        self.n_ctrl = int(n_ctrl)
        self.idx = np.asarray(ctrl_idx, np.uint32)
        self.valid = self.idx != NONE
        self.w = np.where(self.valid, eval_weights(ctrl_kernel, ctrl_sigma, ctrl_d2), F(0)).astype(F)
        self.total = np.zeros(len(self.idx), F)
        for j in range(self.idx.shape[1]):
            self.total = np.where(self.valid[:, j], (self.total + self.w[:, j]).astype(F), self.total)
        reg_idx = np.asarray(reg_idx, np.uint32)
        wr = eval_weights(reg_kernel, reg_sigma, reg_d2)
        s, n, w, directed = [], [], [], []
        for i in range(len(reg_idx)):
            owner = reg_idx[i, 0]
            if owner == NONE:
                continue
            for j in range(1, reg_idx.shape[1]):
                nb = reg_idx[i, j]
                if nb == NONE:
                    continue
                s.append(min(owner, nb)); n.append(max(owner, nb)); w.append(np.sqrt(wr[i, j])); directed.append((int(owner), int(nb)))
        self.arc_s, self.arc_n, self.arc_w = np.array(s, np.int64), np.array(n, np.int64), np.array(w, F)
        self.directed = directed

    def lists(self, sort):
        """(idx, w, valid) per source point in list order, or sorted by node index as the reference leaves them (:1466)"""
        if not sort:
            return self.idx, self.w, self.valid
        order = np.argsort(self.idx, axis=1, kind="stable")      # (NONE is the largest value: padding stays last)
        return np.take_along_axis(self.idx, order, 1), np.take_along_axis(self.w, order, 1), np.take_along_axis(self.valid, order, 1)


# ---- the terms -------------------------------------------------------------------------------------------------------------------
def sqrt_huber(x, delta):
    xa = np.abs(x)
    t = x.dtype.type
    with np.errstate(invalid="ignore"):
        return np.where(xa > delta, np.sqrt(delta * (xa - t(0.5) * delta)), np.sqrt(t(0.5)) * xa)


def sqrt_huber_derivative(x, delta):
    xa = np.abs(x)
    t = x.dtype.type
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(xa > delta, delta / (t(2.0) * np.sqrt(delta * (xa - t(0.5) * delta))), np.sqrt(t(0.5)))
    return np.where(x < 0, -m, m)


def rotation_terms(a, b, c):
    """computeRotationTerms (:38-89) on arrays: four (..., 3, 3) arrays M with M[..., r, c] = the reference's matrix(c, r), i.e. the
    matrices that multiply s (rot^T = Rz(c) Ry(b) Rx(a) and its three derivatives)"""
    sa, ca, sb, cb, sc, cc = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.sin(c), np.cos(c)
    z = np.zeros_like(sa)

    def mat(rows):
        return np.stack([np.stack(r, -1) for r in rows], -2)

    R = mat([[cc * cb, -sc * ca + cc * sb * sa, sc * sa + cc * sb * ca], [sc * cb, cc * ca + sc * sb * sa, -cc * sa + sc * sb * ca], [-sb, cb * sa, cb * ca]])
    Da = mat([[z, sc * sa + cc * sb * ca, sc * ca - cc * sb * sa], [z, -cc * sa + sc * sb * ca, -cc * ca - sc * sb * sa], [z, cb * ca, -cb * sa]])
    Db = mat([[-cc * sb, cc * cb * sa, cc * cb * ca], [-sc * sb, sc * cb * sa, sc * cb * ca], [-cb, -sb * sa, -sb * ca]])
    Dc = mat([[-sc * cb, -cc * ca - sc * sb * sa, cc * sa - sc * sb * ca], [cc * cb, -sc * ca + cc * sb * sa, sc * sa + cc * sb * ca], [z, z, z]])
    return R, Da, Db, Dc


def _mv(M, s):
    """M s, left to right, in the arrays' dtype"""
    return (M[..., 0] * s[..., None, 0] + M[..., 1] * s[..., None, 1]) + M[..., 2] * s[..., None, 2]


def assemble(g, dtype, dst, nrm, src, nn, tf, prm, sort=True):
    """At (6 n_ctrl x equations, CSC), b, and the per-equation bookkeeping: the reference's :1562-1805 for the matched points in ascending
    source order.  Returns (At, b, info) with info = dict(n_pt_eq, n_pl_eq, n_reg_eq, huber_branches)."""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    nn = np.asarray(nn, np.int64)
    m = np.nonzero((nn >= 0) & (nn < len(dst)))[0]
    has_pt, has_pl = len(m) > 0 and prm.w_p2p > 0, len(m) > 0 and prm.w_p2pl > 0
    idx, w, valid = g.lists(sort)
    idx, w, valid = idx[m].astype(np.int64), w[m].astype(t), valid[m]
    idx0 = np.where(valid, idx, 0)
    k = idx.shape[1]
    tot = g.total[m].astype(t)
    ang, tr = np.zeros((len(m), 3), t), np.zeros((len(m), 3), t)
    tf6 = tf.reshape(-1, 6)
    for j in range(k):
        ang = np.where(valid[:, j, None], ang + w[:, j, None] * tf6[idx0[:, j], :3], ang)
        tr = np.where(valid[:, j, None], tr + w[:, j, None] * tf6[idx0[:, j], 3:], tr)
    live = tot != 0
    with np.errstate(all="ignore"):
        inv = np.where(live, t(1.0) / tot, t(1.0))
    ang, tr = ang * inv[:, None], tr * inv[:, None]
    R, Da, Db, Dc = rotation_terms(ang[:, 0], ang[:, 1], ang[:, 2])
    s, d = src[m], dst[nn[m]]
    e = d - (_mv(R, s) + tr)
    da, db, dc = _mv(Da, s), _mv(Db, s), _mv(Dc, s)
    rows, cols, vals, b = [], [], [], []
    n_eq = 0
    unknown = 6 * idx0      # (len(m), k)

    def add(eq, coefs):      # coefs: six (len(m),) arrays, the row's values per unit of weight; weight (len(m), k)
        for c in range(6):
            rows.append((unknown + c)[valid]); cols.append(np.broadcast_to(eq[:, None], unknown.shape)[valid]); vals.append((coefs[c][:, None] * weight)[valid].astype(t))

    n_pt_eq = n_pl_eq = 0
    if has_pt:
        cws = np.where(live, np.sqrt(t(prm.w_p2p)) * np.sqrt(t(1.0)), t(0))
        with np.errstate(all="ignore"):
            cwn = np.where(live, cws / tot, t(0))
        weight = cwn[:, None] * w
        one, zero = np.ones(len(m), t), np.zeros(len(m), t)
        for q in range(3):
            add(3 * np.arange(len(m)) + q, [da[:, q], db[:, q], dc[:, q], one if q == 0 else zero, one if q == 1 else zero, one if q == 2 else zero])
        b.append((e * cws[:, None]).reshape(-1))
        n_pt_eq = 3 * len(m)
        n_eq += n_pt_eq
    if has_pl:
        n = np.asarray(nrm, F).astype(t)[nn[m]]
        cws = np.where(live, np.sqrt(t(prm.w_p2pl)) * np.sqrt(t(1.0)), t(0))
        with np.errstate(all="ignore"):
            cwn = np.where(live, cws / tot, t(0))
        weight = cwn[:, None] * w

        def dot(u, v):
            return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]

        add(n_eq + np.arange(len(m)), [dot(n, da), dot(n, db), dot(n, dc), n[:, 0], n[:, 1], n[:, 2]])
        b.append(dot(n, e) * cws)
        n_pl_eq = len(m)
        n_eq += n_pl_eq
    # regularisation (:1736-1803)
    na = len(g.arc_s)
    wgt = np.sqrt(t(prm.w_reg)) * g.arc_w.astype(t)
    diff = tf6[g.arc_s] - tf6[g.arc_n] if na else np.zeros((0, 6), t)
    hb = t(prm.huber_boundary)
    dh = wgt[:, None] * sqrt_huber_derivative(diff, hb)
    eq = n_eq + 6 * np.arange(na)[:, None] + np.arange(6)[None, :]
    rows += [(6 * g.arc_s[:, None] + np.arange(6)).reshape(-1), (6 * g.arc_n[:, None] + np.arange(6)).reshape(-1)]
    cols += [eq.reshape(-1), eq.reshape(-1)]
    vals += [dh.reshape(-1).astype(t), (-dh).reshape(-1).astype(t)]
    b.append((-wgt[:, None] * sqrt_huber(diff, hb)).reshape(-1))
    n_eq += 6 * na
    At = sp.csc_matrix((np.concatenate(vals).astype(t), (np.concatenate(rows), np.concatenate(cols))), shape=(6 * g.n_ctrl, n_eq), dtype=t)
    info = dict(n_pt_eq=n_pt_eq, n_pl_eq=n_pl_eq, n_reg_eq=6 * na, huber_branches=(bool((np.abs(diff) > hb).any()), bool((np.abs(diff) <= hb).any())), matches=len(m))
    return At, np.concatenate(b).astype(t), info


def assemble_literal(g, dtype, dst, nrm, src, nn, tf, prm):
    """the reference's loops, one row at a time, with the lists sorted by node index (:1456-1469, :1562-1805) -> dense At^T rows as a
    (equations, 6 n_ctrl) array and b"""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    corr = [(int(nn[i]), i) for i in range(len(src)) if 0 <= int(nn[i]) < len(dst)]
    has_pt, has_pl = len(corr) > 0 and prm.w_p2p > 0, len(corr) > 0 and prm.w_p2pl > 0
    lists = []
    for i in range(len(src)):
        lst = [(int(g.idx[i, j]), t(g.w[i, j])) for j in range(g.idx.shape[1]) if g.valid[i, j]]
        lists.append(sorted(lst, key=lambda p: p[0]))
    A, b = [], []

    def data_rows(plane, wsqrt):
        for first, second in corr:
            ang, tr = np.zeros(3, t), np.zeros(3, t)
            for node, wv in lists[second]:
                ang = ang + wv * tf[6 * node:6 * node + 3]
                tr = tr + wv * tf[6 * node + 3:6 * node + 6]
            tot = t(g.total[second])
            if tot != 0:
                wgt = t(1.0) / tot
                ang, tr = ang * wgt, tr * wgt
                cws = wsqrt * np.sqrt(t(1.0))
                cwn = cws / tot
            else:
                cws = cwn = t(0)
            R, Da, Db, Dc = rotation_terms(ang[0:1], ang[1:2], ang[2:3])
            s, d = src[second][None], dst[first][None]
            e = (d - (_mv(R, s) + tr))[0]
            da, db, dc = _mv(Da, s)[0], _mv(Db, s)[0], _mv(Dc, s)[0]
            if plane:
                n = np.asarray(nrm, F).astype(t)[first]
                dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]      # noqa: E731
                row = np.zeros(6 * g.n_ctrl, t)
                for node, wv in lists[second]:
                    weight = cwn * wv
                    row[6 * node:6 * node + 6] += np.array([dot(n, da) * weight, dot(n, db) * weight, dot(n, dc) * weight, n[0] * weight, n[1] * weight, n[2] * weight], t)
                A.append(row); b.append(dot(n, e) * cws)
            else:
                for q in range(3):
                    row = np.zeros(6 * g.n_ctrl, t)
                    for node, wv in lists[second]:
                        weight = cwn * wv
                        unit = [weight if q == r else t(0) for r in range(3)]
                        row[6 * node:6 * node + 6] += np.array([da[q] * weight, db[q] * weight, dc[q] * weight] + unit, t)
                    A.append(row); b.append(e[q] * cws)

    if has_pt:
        data_rows(False, np.sqrt(t(prm.w_p2p)))
    if has_pl:
        data_rows(True, np.sqrt(t(prm.w_p2pl)))
    hb = t(prm.huber_boundary)
    for (owner, nb), aw in zip(g.directed, g.arc_w):
        s_off, n_off = 6 * owner, 6 * nb
        weight = np.sqrt(t(prm.w_reg)) * t(aw)
        if n_off < s_off:
            s_off, n_off = n_off, s_off
        for c in range(6):
            diff = np.array([tf[s_off + c] - tf[n_off + c]], t)
            dh = weight * sqrt_huber_derivative(diff, hb)[0]
            row = np.zeros(6 * g.n_ctrl, t)
            row[s_off + c] += dh; row[n_off + c] += -dh
            A.append(row); b.append(-weight * sqrt_huber(diff, hb)[0])
    return np.array(A, t).reshape(len(A), 6 * g.n_ctrl), np.array(b, t)


def assemble_dense_literal(dtype, dst, nrm, src, nn, reg_idx, reg_w_sqrt, tf, prm):
    """the DENSE estimator's system (:488-700): one unknown block per source point, weight = sqrt(metric weight) with no total -> (A, b)"""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    corr = [(int(nn[i]), i) for i in range(len(src)) if 0 <= int(nn[i]) < len(dst)]
    A, b = [], []
    nu = 6 * len(src)
    for plane, on, wsqrt in ((False, prm.w_p2p > 0, np.sqrt(t(prm.w_p2p))), (True, prm.w_p2pl > 0, np.sqrt(t(prm.w_p2pl)))):
        if not on or not corr:
            continue
        for first, second in corr:
            off = 6 * second
            weight = wsqrt * np.sqrt(t(1.0))
            R, Da, Db, Dc = rotation_terms(tf[off:off + 1], tf[off + 1:off + 2], tf[off + 2:off + 3])
            s, d = src[second][None], dst[first][None]
            e = (d - (_mv(R, s) + tf[off + 3:off + 6]))[0]
            da, db, dc = _mv(Da, s)[0], _mv(Db, s)[0], _mv(Dc, s)[0]
            if plane:
                n = np.asarray(nrm, F).astype(t)[first]
                dot = lambda u, v: (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]      # noqa: E731
                row = np.zeros(nu, t)
                row[off:off + 6] = [dot(n, da) * weight, dot(n, db) * weight, dot(n, dc) * weight, n[0] * weight, n[1] * weight, n[2] * weight]
                A.append(row); b.append(dot(n, e) * weight)
            else:
                for q in range(3):
                    row = np.zeros(nu, t)
                    row[off:off + 3] = [da[q] * weight, db[q] * weight, dc[q] * weight]
                    row[off + 3 + q] = weight
                    A.append(row); b.append(e[q] * weight)
    hb = t(prm.huber_boundary)
    for i in range(len(reg_idx)):
        for j in range(1, reg_idx.shape[1]):
            if reg_idx[i, 0] == NONE or reg_idx[i, j] == NONE:
                continue
            s_off, n_off = 6 * int(reg_idx[i, 0]), 6 * int(reg_idx[i, j])
            weight = np.sqrt(t(prm.w_reg)) * t(reg_w_sqrt[i, j])
            if n_off < s_off:
                s_off, n_off = n_off, s_off
            for c in range(6):
                diff = np.array([tf[s_off + c] - tf[n_off + c]], t)
                dh = weight * sqrt_huber_derivative(diff, hb)[0]
                row = np.zeros(nu, t)
                row[s_off + c] += dh; row[n_off + c] += -dh
                A.append(row); b.append(-weight * sqrt_huber(diff, hb)[0])
    return np.array(A, t).reshape(len(A), nu), np.array(b, t)


def apply_matrix_free(At, p):
    """(A^T A) p as the device forms it: u = A p per row, then A^T u per unknown (no product matrix)"""
    return At @ (At.T @ p)


# ---- Eigen's conjugate_gradient() with the diagonal preconditioner, x0 = 0 ------------------------------------------------------------
def eigen_cg(mat, rhs, tol, max_iter, dtype):
    """-> (x, iterations, |residual|^2 of the recurrence).  mat: anything with @ and .diagonal()"""
    t = dtype
    rhs = np.asarray(rhs, t)
    diag = np.asarray(mat.diagonal(), t)
    with np.errstate(all="ignore"):
        inv = np.where(diag != 0, t(1.0) / diag, t(1.0)).astype(t)
    x = np.zeros(len(rhs), t)
    residual = rhs.copy()
    rhs2 = t(np.dot(rhs, rhs))
    if rhs2 == 0:
        return x, 0, t(0)
    threshold = max(t(t(tol) * t(tol) * rhs2), t(np.finfo(np.float32).tiny if t is np.float32 else np.finfo(np.float64).tiny))
    res2 = t(np.dot(residual, residual))
    if res2 < threshold:
        return x, 0, res2
    p = (inv * residual).astype(t)
    abs_new = t(np.dot(residual, p))
    i = 0
    while i < max_iter:
        tmp = np.asarray(mat @ p, t)
        alpha = t(abs_new / t(np.dot(p, tmp)))
        x = (x + alpha * p).astype(t)
        residual = (residual - alpha * tmp).astype(t)
        res2 = t(np.dot(residual, residual))
        if res2 < threshold:
            break
        z = (inv * residual).astype(t)
        abs_old = abs_new
        abs_new = t(np.dot(residual, z))
        beta = t(abs_new / abs_old)
        p = (z + beta * p).astype(t)
        i += 1
    return x, i, res2


def estimate(g, dtype, dst, nrm, src, nn, prm, sort=True, record=None):
    """estimateSparseWarpFieldCombinedMetric -> (tforms_vec, stats).  stats: gn_iterations, converged, cg_iterations_total,
    last_cg_residual_norm2, max_delta_sq, data_term.  record: a list that receives (At, b, AtA, Atb, delta, cg iterations) per step."""
    t = dtype
    tf = np.zeros(6 * g.n_ctrl, t)
    nn = np.asarray(nn, np.int64)
    matches = int(((nn >= 0) & (nn < len(dst))).sum())
    st = dict(gn_iterations=0, converged=False, cg_iterations_total=0, last_cg_residual_norm2=0.0, max_delta_sq=0.0, data_term=True, huber_branches=[False, False])
    if matches == 0 or not (prm.w_p2p > 0 or prm.w_p2pl > 0):      # (:1427-1433)
        st["data_term"] = False
        return tf, st
    while st["gn_iterations"] < prm.max_gn_iter:
        At, b, info = assemble(g, t, dst, nrm, src, nn, tf, prm, sort)
        AtA = (At @ At.T).tocsc()
        Atb = np.asarray(At @ b, t)
        delta, its, res2 = eigen_cg(AtA, Atb, prm.cg_conv_tol, prm.max_cg_iter, t)
        if record is not None:
            record.append((At, b, AtA, Atb, delta, its))
        tf = (tf + delta).astype(t)
        st["gn_iterations"] += 1
        st["cg_iterations_total"] += its
        st["last_cg_residual_norm2"] = float(res2)
        st["huber_branches"] = [st["huber_branches"][q] or info["huber_branches"][q] for q in range(2)]
        d6 = delta.reshape(-1, 6)
        st["max_delta_sq"] = float((d6 * d6).sum(1).max())
        if t(st["max_delta_sq"]) < t(prm.gn_conv_tol) * t(prm.gn_conv_tol):
            st["converged"] = True
            break
    return tf, st


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def polish(L):
    """LinearTransform::rotation() (space_transformations.hpp:43-51) on (..., 3, 3) arrays, in their dtype"""
    U, _, Vt = np.linalg.svd(L)
    neg = np.linalg.det(U @ Vt) < 0
    U = U.copy()
    U[neg, :, 0] *= -1
    return (U @ Vt).astype(L.dtype)


def to_transforms(tf, dtype):
    """(a, b, c, t) per node -> Rz(c) Ry(b) Rx(a) through rotation(), translation t (:1833-1843)"""
    tf6 = np.asarray(tf).astype(dtype).reshape(-1, 6)
    R = rotation_terms(tf6[:, 0], tf6[:, 1], tf6[:, 2])[0]
    T = np.zeros((len(tf6), 4, 4), dtype)
    T[:, :3, :3] = polish(R)
    T[:, :3, 3] = tf6[:, 3:]
    T[:, 3, 3] = 1
    return T


def angles_of(T):
    """(a, b, c) of R = Rz(c) Ry(b) Rx(a), f64"""
    T = np.asarray(T, np.float64)
    return np.stack([np.arctan2(T[:, 2, 1], T[:, 2, 2]), -np.arcsin(np.clip(T[:, 2, 0], -1, 1)), np.arctan2(T[:, 1, 0], T[:, 0, 0])], 1)


def resample(g, ctrl_T, dtype):
    """resampleTransforms, the list overload (warp_field_utilities.hpp:14-48), in list order"""
    t = dtype
    ctrl_T = np.asarray(ctrl_T).astype(t)
    n, k = g.idx.shape
    M = np.zeros((n, 3, 4), t)
    idx0 = np.where(g.valid, g.idx, 0).astype(np.int64)
    w = g.w.astype(t)
    for j in range(k):
        M = np.where(g.valid[:, j, None, None], M + w[:, j, None, None] * ctrl_T[idx0[:, j], :3, :], M)
    tot = g.total.astype(t)
    out = np.tile(np.eye(4, dtype=t), (n, 1, 1))
    live = tot != 0
    with np.errstate(all="ignore"):
        inv = t(1.0) / tot[live]
    out[live, :3, :3] = polish((M[live, :, :3] * inv[:, None, None]).astype(t))
    out[live, :3, 3] = M[live, :, 3] * inv[:, None]
    return out


def transform_points(T, xyz):
    """out_i = ((L0 x + L1 y) + L2 z) + t in f32, every operation rounded once"""
    T, p = np.asarray(T, F), np.asarray(xyz, F)
    return (((T[:, :3, 0] * p[:, None, 0] + T[:, :3, 1] * p[:, None, 1]) + T[:, :3, 2] * p[:, None, 2]) + T[:, :3, 3]).astype(F)


def compose(T_iter, T, dtype):
    """T[i] = T_iter[i] * T[i]; -> (T, max_i |R_iter - I|_F^2 + |t_iter|^2)"""
    A, B = np.asarray(T_iter).astype(dtype), np.asarray(T).astype(dtype)
    out = (A @ B).astype(dtype)
    out[:, 3, :] = [0, 0, 0, 1]
    d = A[:, :3, :3] - np.eye(3, dtype=dtype)
    return out, float(((d * d).sum((1, 2)) + (A[:, :3, 3] ** 2).sum(1)).max())


def plane_residuals(dst, nrm, q):
    """per point of q: |n . (d - q)| against its nearest target point (no distance limit)"""
    nn = nearest(dst, q, np.inf).astype(np.int64)
    return np.abs(((np.asarray(dst, np.float64)[nn] - np.asarray(q, np.float64)) * np.asarray(nrm, np.float64)[nn]).sum(1))


def icp_loop(g, dtype, dst, nrm, src, prm, max_iter, conv_tol, max_sq, sort=True):
    """icp_base.hpp:68-87 over icp_warp_field_combined_metric_sparse.hpp:202-240 -> dict(T, dense, iterations, last_delta_norm, ncorr (per
    iteration), near_threshold (per iteration: matches whose d2 is within `band` of max_sq), warped)"""
    t = dtype
    T = np.tile(np.eye(4, dtype=t), (g.n_ctrl, 1, 1))
    dense = resample(g, T, t)
    its, last, ncorr = 0, np.inf, []
    warped = transform_points(dense, src)
    while its < max_iter:
        warped = transform_points(dense, src)
        nn = nearest(dst, warped, max_sq)
        ncorr.append(int((nn != NONE).sum()))
        tf, _ = estimate(g, t, dst, nrm, warped, np.where(nn == NONE, -1, nn.astype(np.int64)), prm, sort)
        T, d2 = compose(to_transforms(tf, t), T, t)
        dense = resample(g, T, t)
        last = float(np.sqrt(t(d2)))
        its += 1
        if last < conv_tol:
            break
    return dict(T=T, dense=dense, iterations=its, last_delta_norm=last, ncorr=ncorr, warped=transform_points(dense, src))


# ---- the test clouds ---------------------------------------------------------------------------------------------------------------
def control_nodes(points, res):
    """voxel-grid centroids (what gridDownsample gives), in ascending cell order"""
    p = np.asarray(points, np.float64)
    cell = np.floor(p / res).astype(np.int64)
    _, inv = np.unique(cell, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv)
    return np.stack([np.bincount(inv, p[:, c]) / cnt for c in range(3)], 1).astype(F)


def make_case(n_src=3000, n_dst=4000, res=0.07, k_ctrl=4, k_reg=8, amplitude=0.004, ctrl_kernel=RBF, reg_kernel=RBF, ctrl_sigma=None, reg_sigma=None):
    """the tests' cloud pair: a curved surface sampled twice (cilantro_amd/synthetic.py), the target bent by a smooth displacement of a few
    millimetres; control nodes = voxel-grid centroids of the source at `res`; the example's sigmas (0.5 res, 3 res) unless given"""
    from cilantro_amd import synthetic

    src, _ = synthetic.make_surface(n_src, seed=45)
    flat, dst_n = synthetic.make_surface(n_dst, seed=46)
    dst = synthetic.bend(flat, amplitude)
    ctrl = control_nodes(src, res)
    ctrl_idx, ctrl_d2 = knn_lists(ctrl, src, k_ctrl)
    reg_idx, reg_d2 = knn_lists(ctrl, ctrl, k_reg)
    cs, rs = F(0.5 * res if ctrl_sigma is None else ctrl_sigma), F(3.0 * res if reg_sigma is None else reg_sigma)
    g = Graph(len(ctrl), ctrl_idx, ctrl_d2, ctrl_kernel, cs, reg_idx, reg_d2, reg_kernel, rs)
    return dict(src=src, dst=dst, dst_n=dst_n, ctrl=ctrl, ctrl_idx=ctrl_idx, ctrl_d2=ctrl_d2, reg_idx=reg_idx, reg_d2=reg_d2, n_ctrl=len(ctrl), graph=g, ctrl_kernel=ctrl_kernel,
                reg_kernel=reg_kernel, ctrl_sigma=cs, reg_sigma=rs, res=res, max_sq=F((0.8 * res) ** 2))


# ---- a graph that scales: lists from a lattice, no all-pairs temporary -----------------------------------------------------------
def d2_pairs(q, p):
    """d2_pinned for aligned pairs: (dx dx + dy dy) + dz dz in f32, element i of q against element i of p"""
    d = np.asarray(q, F) - np.asarray(p, F)
    return ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).astype(F)


def surface(x, y):
    """the height field of cilantro_amd/synthetic.py make_surface (extent 1) at given x, y, f64 -> (z, unit normals)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    k1, k2 = 2.0 * np.pi * 0.8, 2.0 * np.pi * 0.6
    z = 0.12 * np.sin(k1 * x) * np.cos(k2 * y) + 0.05 * np.cos(1.7 * k1 * x + 0.9 * k2 * y)
    zx = 0.12 * k1 * np.cos(k1 * x) * np.cos(k2 * y) - 0.05 * 1.7 * k1 * np.sin(1.7 * k1 * x + 0.9 * k2 * y)
    zy = -0.12 * k2 * np.sin(k1 * x) * np.sin(k2 * y) - 0.05 * 0.9 * k2 * np.sin(1.7 * k1 * x + 0.9 * k2 * y)
    n = np.stack([-zx, -zy, np.ones_like(z)], -1)
    return z, n / np.linalg.norm(n, axis=-1, keepdims=True)


def lattice_offsets(count):
    """the first `count` lattice steps (dx, dy) != (0, 0) by ascending dx^2 + dy^2, then dy, then dx: the 4-neighbourhood, the diagonals, ..."""
    r = int(np.ceil(np.sqrt(count))) + 1      # (the disc of this radius holds more than `count` steps and lies inside the window)
    steps = sorted(((dx * dx + dy * dy, dy, dx) for dx in range(-r, r + 1) for dy in range(-r, r + 1) if dx or dy))
    return [(dx, dy) for _, dy, dx in steps[:count]]


def lattice_reg_lists(nx, ny, k_reg, ctrl):
    """row i = [i, the lattice neighbours of node i in the order of lattice_offsets...], padded with NONE where the lattice ends (ragged
    at the border); d2 through the pinned expression for the listed pairs only"""
    n = nx * ny
    ix, iy = np.arange(n) % nx, np.arange(n) // nx
    idx = np.full((n, k_reg), NONE, np.uint32)
    idx[:, 0] = np.arange(n)
    fill = np.ones(n, np.int64)
    for dx, dy in lattice_offsets(k_reg - 1):
        jx, jy = ix + dx, iy + dy
        ok = (jx >= 0) & (jx < nx) & (jy >= 0) & (jy < ny)
        idx[np.nonzero(ok)[0], fill[ok]] = (jy * nx + jx)[ok]
        fill[ok] += 1
    d2 = np.zeros((n, k_reg), F)
    live = idx != NONE
    rows = np.broadcast_to(np.arange(n)[:, None], idx.shape)
    d2[live] = d2_pairs(ctrl[rows[live]], ctrl[idx[live].astype(np.int64)])
    return idx, d2


def nearest_node_lists(ctrl, pts, k):
    """knn_lists(ctrl, pts, k) without the all-pairs temporary: candidates from a k-d tree over the nodes, ordered by the pinned f32 d2,
    ties by lowest index.  (The tree works in f64: it hands over k + 6 candidates, so a pair of near-equal distances that f32 orders
    the other way is still inside.)"""
    from scipy.spatial import cKDTree

    ctrl, pts = np.asarray(ctrl, F), np.asarray(pts, F)
    kq = min(len(ctrl), k + 6)
    cand = cKDTree(ctrl.astype(np.float64)).query(pts.astype(np.float64), k=kq)[1].reshape(len(pts), kq).astype(np.int64)
    dd = d2_pairs(pts[:, None, :], ctrl[cand])
    order = np.lexsort((cand, dd), axis=1)[:, :k]
    kk = order.shape[1]
    idx, d2 = np.full((len(pts), k), NONE, np.uint32), np.zeros((len(pts), k), F)
    idx[:, :kk], d2[:, :kk] = np.take_along_axis(cand, order, 1), np.take_along_axis(dd, order, 1)
    return idx, d2


def make_lattice_case(nx, ny, k_ctrl, k_reg, extra=0, seed=0, amplitude=0.004, ctrl_kernel=RBF, reg_kernel=RBF, jitter=0.3, unmatched_every=11):
    """make_case's dict for an nx x ny lattice of control nodes on the same curved surface (spacing h = 1 / max(nx, ny), node i at column
    i % nx, row i // nx), in time and memory linear in the sizes.  The lists are input data to cilhip_warp_field_create and need not be
    a k-NN of anything: the regularisation rows are the lattice neighbourhoods (lattice_reg_lists), the control lists each source
    point's k_ctrl nearest nodes (nearest_node_lists).  Source: the nodes moved by up to jitter h in x and y (and 0.05 h off the
    surface), then `extra` points spread over the lattice's extent.  Target: one point per source point, 0.2 h away in x and y on the
    surface, bent by `amplitude`, with the surface's normal; nn[i] = i except every `unmatched_every`-th from 5 on, which is NONE (the
    correspondences are data too).  Sigmas as the example's: 0.5 h and 3 h."""
    from cilantro_amd import synthetic

    n = nx * ny
    h = 1.0 / max(nx, ny)
    rng = np.random.RandomState(seed)
    gx, gy = (np.arange(n) % nx + 0.5) * h, (np.arange(n) // nx + 0.5) * h
    ctrl = np.stack([gx, gy, surface(gx, gy)[0]], 1).astype(F)
    sx = np.concatenate([gx + jitter * h * rng.uniform(-1, 1, n), rng.uniform(0, nx * h, extra)])
    sy = np.concatenate([gy + jitter * h * rng.uniform(-1, 1, n), rng.uniform(0, ny * h, extra)])
    src = np.stack([sx, sy, surface(sx, sy)[0] + 0.05 * h * rng.uniform(-1, 1, len(sx))], 1).astype(F)
    tx, ty = sx + 0.2 * h * rng.uniform(-1, 1, len(sx)), sy + 0.2 * h * rng.uniform(-1, 1, len(sx))
    tz, dst_n = surface(tx, ty)
    dst = synthetic.bend(np.stack([tx, ty, tz], 1).astype(F), amplitude)
    nn = np.arange(len(src), dtype=np.uint32)
    if unmatched_every:
        nn[5::unmatched_every] = NONE
    ctrl_idx, ctrl_d2 = nearest_node_lists(ctrl, src, k_ctrl)
    reg_idx, reg_d2 = lattice_reg_lists(nx, ny, k_reg, ctrl)
    cs, rs = F(0.5 * h), F(3.0 * h)
    g = Graph(n, ctrl_idx, ctrl_d2, ctrl_kernel, cs, reg_idx, reg_d2, reg_kernel, rs)
    return dict(src=src, dst=dst, dst_n=np.ascontiguousarray(dst_n, F), ctrl=ctrl, ctrl_idx=ctrl_idx, ctrl_d2=ctrl_d2, reg_idx=reg_idx, reg_d2=reg_d2, n_ctrl=n, graph=g,
                ctrl_kernel=ctrl_kernel, reg_kernel=reg_kernel, ctrl_sigma=cs, reg_sigma=rs, res=F(h), max_sq=F((3.0 * h) ** 2), nn=nn, nx=nx, ny=ny)
