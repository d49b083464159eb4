"""numpy / scipy restatement of DESIGN.md section 17.4 (the warp field with AFFINE node transforms), the yardstick of
tests/test_gpu_warp_field_affine.py.

The reference's estimator (registration/warp_field_estimation.hpp:1859-2234, the dense one :725-1005) is restated the way it runs, as
tests/_warp_refs.py restates the rigid one; the graph, the weights, the totals, the arcs (W1), Eigen's CG (W5), the no-data case (W8)
and the per-point transform (W9) ARE that module's and are imported from it.  What differs is stated here:
  A1  tforms_vec holds 12 values per node, the 3 x 3 linear part row-major, then t; the start is the identity and t = 0
  A2  the blend of the 12 values in list order, scaled by the RECIPROCAL of the total; s_t = (L s) + tr
  A3  the rows: the linear part's coefficients carry s_t, not s -- the reference as written (:2091, :2153).  `jac_point="s"` builds
      the variant with the true Jacobian; it exists so that the tests can show that the device reproduces the reference, not the fix
  A4  twelve rows per arc            A5  |delta_node|^2 over 12 components
  A6  no rotation() on the way out   A7  the resample is the plain blend

Every function takes a dtype: np.float32 is "the reference as it runs", np.float64 "the exact answer".
Layouts: transforms are (n, 4, 4) arrays T[i][r, c]; tforms_vec is (12 n_ctrl,)."""
import numpy as np
import scipy.sparse as sp

import _warp_refs as W
from _warp_refs import F, NONE, Graph, eigen_cg, make_case, nearest, sqrt_huber, sqrt_huber_derivative, transform_points  # noqa: F401

NU = 12


def identity_start(n_ctrl, dtype):
    tf = np.zeros((n_ctrl, NU), dtype)
    tf[:, [0, 4, 8]] = 1
    return tf.reshape(-1)


def _dot3(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def blend(g, dtype, tf, m, sort=True):
    """A2 for the source points m -> (lin (len(m), 9), tr (len(m), 3), idx0, w, valid, total), in the dtype"""
    t = dtype
    idx, w, valid = g.lists(sort)
    idx, w, valid = idx[m].astype(np.int64), w[m].astype(t), valid[m]
    idx0 = np.where(valid, idx, 0)
    tot = g.total[m].astype(t)
    tf12 = np.asarray(tf).astype(t).reshape(-1, NU)
    lin, tr = np.zeros((len(m), 9), t), np.zeros((len(m), 3), t)
    for j in range(idx.shape[1]):
        lin = np.where(valid[:, j, None], lin + w[:, j, None] * tf12[idx0[:, j], :9], lin)
        tr = np.where(valid[:, j, None], tr + w[:, j, None] * tf12[idx0[:, j], 9:], tr)
    live = tot != 0
    with np.errstate(all="ignore"):
        inv = np.where(live, t(1.0) / tot, t(1.0))      # (left unscaled where the total is 0: :2059)
    return (lin * inv[:, None]).astype(t), (tr * inv[:, None]).astype(t), idx0, w, valid, tot


def assemble(g, dtype, dst, nrm, src, nn, tf, prm, sort=True, jac_point="s_t"):
    """At (12 n_ctrl x equations, CSC), b, info: the reference's :2043-2194 for the matched points in ascending source order"""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    nn = np.asarray(nn, np.int64)
    m = np.nonzero((nn >= 0) & (nn < len(dst)))[0]
    has_pt, has_pl = len(m) > 0 and prm.w_p2p > 0, len(m) > 0 and prm.w_p2pl > 0
    lin, tr, idx0, w, valid, tot = blend(g, t, tf, m, sort)
    live = tot != 0
    s, d = src[m], dst[nn[m]]
    s_t = (W._mv(lin.reshape(-1, 3, 3), s) + tr).astype(t)
    e = d - s_t
    jp = s_t if jac_point == "s_t" else s
    rows, cols, vals, b = [], [], [], []
    unknown = NU * idx0
    n_eq = n_pt_eq = n_pl_eq = 0

    def put(eq, c, value):      # one coefficient per (point, slot): value (len(m), k) at unknown c of the slot's node
        rows.append((unknown + c)[valid]); cols.append(np.broadcast_to(eq[:, None], unknown.shape)[valid]); vals.append(value[valid].astype(t))

    def weights(metric_w):
        cws = np.where(live, np.sqrt(t(metric_w)) * np.sqrt(t(1.0)), t(0))
        with np.errstate(all="ignore"):
            cwn = np.where(live, cws / tot, t(0))
        return cws, cwn[:, None] * w

    if has_pt:
        cws, weight = weights(prm.w_p2p)
        for q in range(3):
            eq = 3 * np.arange(len(m)) + q
            for nz in range(3):
                put(eq, 3 * q + nz, weight * jp[:, nz, None])
            put(eq, 9 + q, weight)
        b.append((cws[:, None] * e).reshape(-1))
        n_pt_eq = 3 * len(m)
        n_eq += n_pt_eq
    if has_pl:
        n = np.asarray(nrm, F).astype(t)[nn[m]]
        cws, weight = weights(prm.w_p2pl)
        eq = n_eq + np.arange(len(m))
        for blk in range(3):
            for cur in range(3):
                put(eq, 3 * blk + cur, (weight * n[:, blk, None]) * jp[:, cur, None])
        for cur in range(3):
            put(eq, 9 + cur, weight * n[:, cur, None])
        b.append(_dot3(n, e) * cws)
        n_pl_eq = len(m)
        n_eq += n_pl_eq
    na = len(g.arc_s)
    tf12 = tf.reshape(-1, NU)
    wgt = np.sqrt(t(prm.w_reg)) * g.arc_w.astype(t)
    diff = tf12[g.arc_s] - tf12[g.arc_n] if na else np.zeros((0, NU), t)
    hb = t(prm.huber_boundary)
    dh = wgt[:, None] * sqrt_huber_derivative(diff, hb)
    eq = n_eq + NU * np.arange(na)[:, None] + np.arange(NU)[None, :]
    rows += [(NU * g.arc_s[:, None] + np.arange(NU)).reshape(-1), (NU * g.arc_n[:, None] + np.arange(NU)).reshape(-1)]
    cols += [eq.reshape(-1), eq.reshape(-1)]
    vals += [dh.reshape(-1).astype(t), (-dh).reshape(-1).astype(t)]
    b.append((-wgt[:, None] * sqrt_huber(diff, hb)).reshape(-1))
    n_eq += NU * na
    At = sp.csc_matrix((np.concatenate(vals).astype(t), (np.concatenate(rows), np.concatenate(cols))), shape=(NU * g.n_ctrl, n_eq), dtype=t)
    info = dict(n_pt_eq=n_pt_eq, n_pl_eq=n_pl_eq, n_reg_eq=NU * na, huber_branches=(bool((np.abs(diff) > hb).any()), bool((np.abs(diff) <= hb).any())), matches=len(m),
                s=s, s_t=s_t, points=m)
    return At, np.concatenate(b).astype(t), info


def _arc_rows_literal(A, b, t, pairs, weights, tf, prm, nu_total):
    hb = t(prm.huber_boundary)
    for (owner, nb), aw in zip(pairs, weights):
        s_off, n_off = NU * owner, NU * nb
        weight = np.sqrt(t(prm.w_reg)) * t(aw)
        if n_off < s_off:
            s_off, n_off = n_off, s_off
        for c in range(NU):
            diff = np.array([tf[s_off + c] - tf[n_off + c]], t)
            dh = weight * sqrt_huber_derivative(diff, hb)[0]
            row = np.zeros(nu_total, t)
            row[s_off + c] += dh; row[n_off + c] += -dh
            A.append(row); b.append(-weight * sqrt_huber(diff, hb)[0])


def assemble_literal(g, dtype, dst, nrm, src, nn, tf, prm):
    """the reference's loops (:2043-2194), one row at a time, with the lists sorted by node index -> dense (equations, 12 n_ctrl), b"""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    corr = [(int(nn[i]), i) for i in range(len(src)) if 0 <= int(nn[i]) < len(dst)]
    has_pt, has_pl = len(corr) > 0 and prm.w_p2p > 0, len(corr) > 0 and prm.w_p2pl > 0
    lists = []
    for i in range(len(src)):
        lst = [(int(g.idx[i, j]), t(g.w[i, j])) for j in range(g.idx.shape[1]) if g.valid[i, j]]
        lists.append(sorted(lst, key=lambda p: p[0]))
    A, b = [], []
    nu_total = NU * g.n_ctrl

    def data_rows(plane, wsqrt):
        for first, second in corr:
            lin, tr = np.zeros(9, t), np.zeros(3, t)
            for node, wv in lists[second]:
                lin = lin + wv * tf[NU * node:NU * node + 9]
                tr = tr + wv * tf[NU * node + 9:NU * node + 12]
            tot = t(g.total[second])
            if tot != 0:
                wgt = t(1.0) / tot
                lin, tr = lin * wgt, tr * wgt
                cws = wsqrt * np.sqrt(t(1.0))
                cwn = cws / tot
            else:
                cws = cwn = t(0)
            s, d = src[second], dst[first]
            L = lin.reshape(3, 3)
            s_t = np.array([((L[r, 0] * s[0] + L[r, 1] * s[1]) + L[r, 2] * s[2]) + tr[r] for r in range(3)], t)
            if plane:
                n = np.asarray(nrm, F).astype(t)[first]
                row = np.zeros(nu_total, t)
                for node, wv in lists[second]:
                    weight = cwn * wv
                    for blk in range(3):
                        for cur in range(3):
                            row[NU * node + 3 * blk + cur] += weight * n[blk] * s_t[cur]
                    for cur in range(3):
                        row[NU * node + 9 + cur] += weight * n[cur]
                A.append(row); b.append(_dot3(n, d - s_t) * cws)
            else:
                rws = [np.zeros(nu_total, t) for _ in range(3)]
                for node, wv in lists[second]:
                    weight = cwn * wv
                    for eq in range(3):
                        for nz in range(3):
                            rws[eq][NU * node + 3 * eq + nz] += weight * s_t[nz]
                        rws[eq][NU * node + 9 + eq] += weight
                A.extend(rws); b.extend(list(cws * (d - s_t)))

    if has_pt:
        data_rows(False, np.sqrt(t(prm.w_p2p)))
    if has_pl:
        data_rows(True, np.sqrt(t(prm.w_p2pl)))
    _arc_rows_literal(A, b, t, g.directed, g.arc_w, tf, prm, nu_total)
    return np.array(A, t).reshape(len(A), nu_total), np.array(b, t)


def assemble_dense_literal(dtype, dst, nrm, src, nn, reg_idx, reg_w_sqrt, tf, prm):
    """the DENSE affine estimator's system (:856-955): one unknown block per source point, weight = sqrt(metric weight), no total"""
    t = dtype
    dst, src, tf = np.asarray(dst, F).astype(t), np.asarray(src, F).astype(t), np.asarray(tf).astype(t)
    corr = [(int(nn[i]), i) for i in range(len(src)) if 0 <= int(nn[i]) < len(dst)]
    A, b = [], []
    nu_total = NU * len(src)
    for plane, on, wsqrt in ((False, prm.w_p2p > 0, np.sqrt(t(prm.w_p2p))), (True, prm.w_p2pl > 0, np.sqrt(t(prm.w_p2pl)))):
        if not on or not corr:
            continue
        for first, second in corr:
            off = NU * second
            weight = wsqrt * np.sqrt(t(1.0))
            L, tr = tf[off:off + 9].reshape(3, 3), tf[off + 9:off + 12]
            s, d = src[second], dst[first]
            s_t = np.array([((L[r, 0] * s[0] + L[r, 1] * s[1]) + L[r, 2] * s[2]) + tr[r] for r in range(3)], t)
            if plane:
                n = np.asarray(nrm, F).astype(t)[first]
                row = np.zeros(nu_total, t)
                for blk in range(3):
                    for cur in range(3):
                        row[off + 3 * blk + cur] = weight * n[blk] * s_t[cur]
                for cur in range(3):
                    row[off + 9 + cur] = weight * n[cur]
                A.append(row); b.append(_dot3(n, d - s_t) * weight)
            else:
                for eq in range(3):
                    row = np.zeros(nu_total, t)
                    for nz in range(3):
                        row[off + 3 * eq + nz] = weight * s_t[nz]
                    row[off + 9 + eq] = weight
                    A.append(row); b.append(weight * (d - s_t)[eq])
    pairs, ws = [], []
    for i in range(len(reg_idx)):
        for j in range(1, reg_idx.shape[1]):
            if reg_idx[i, 0] == NONE or reg_idx[i, j] == NONE:
                continue
            pairs.append((int(reg_idx[i, 0]), int(reg_idx[i, j]))); ws.append(reg_w_sqrt[i, j])
    _arc_rows_literal(A, b, t, pairs, ws, tf, prm, nu_total)
    return np.array(A, t).reshape(len(A), nu_total), np.array(b, t)


def estimate(g, dtype, dst, nrm, src, nn, prm, sort=True, record=None, jac_point="s_t"):
    """the affine estimateSparseWarpFieldCombinedMetric -> (tforms_vec, stats), the statistics of _warp_refs.estimate"""
    t = dtype
    tf = identity_start(g.n_ctrl, t)
    nn = np.asarray(nn, np.int64)
    matches = int(((nn >= 0) & (nn < len(dst))).sum())
    st = dict(gn_iterations=0, converged=False, cg_iterations_total=0, last_cg_residual_norm2=0.0, max_delta_sq=0.0, data_term=True, huber_branches=[False, False])
    if matches == 0 or not (prm.w_p2p > 0 or prm.w_p2pl > 0):      # (W8)
        st["data_term"] = False
        return tf, st
    while st["gn_iterations"] < prm.max_gn_iter:
        At, b, info = assemble(g, t, dst, nrm, src, nn, tf, prm, sort, jac_point)
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
        d12 = delta.reshape(-1, NU)
        st["max_delta_sq"] = float((d12 * d12).sum(1).max())
        if t(st["max_delta_sq"]) < t(prm.gn_conv_tol) * t(prm.gn_conv_tol):
            st["converged"] = True
            break
    return tf, st


# ---- transforms ------------------------------------------------------------------------------------------------------------------
def to_transforms(tf, dtype):
    """A6: the linear part and the translation as they are"""
    tf12 = np.asarray(tf).astype(dtype).reshape(-1, NU)
    T = np.zeros((len(tf12), 4, 4), dtype)
    T[:, :3, :3] = tf12[:, :9].reshape(-1, 3, 3)
    T[:, :3, 3] = tf12[:, 9:]
    T[:, 3, 3] = 1
    return T


def readback(T):
    """(L row-major, t) per node, f64, from transforms"""
    T = np.asarray(T, np.float64)
    return np.concatenate([T[:, :3, :3].reshape(len(T), 9), T[:, :3, 3]], 1)


def resample(g, ctrl_T, dtype):
    """A7: T_i = (sum_j w_ij T_j) * (1 / total_i) in list order, no polish; the identity where total_i == 0"""
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
    out[live, :3, :] = M[live] * inv[:, None, None]
    return out


def icp_loop(g, dtype, dst, nrm, src, prm, max_iter, conv_tol, max_sq, sort=True):
    """A8: _warp_refs.icp_loop with A6 / A7 in place of W7 / W9"""
    t = dtype
    T = np.tile(np.eye(4, dtype=t), (g.n_ctrl, 1, 1))
    dense = resample(g, T, t)
    its, last, ncorr = 0, np.inf, []
    while its < max_iter:
        warped = transform_points(dense, src)
        nn = nearest(dst, warped, max_sq)
        ncorr.append(int((nn != NONE).sum()))
        tf, _ = estimate(g, t, dst, nrm, warped, np.where(nn == NONE, -1, nn.astype(np.int64)), prm, sort)
        T, d2 = W.compose(to_transforms(tf, t), T, t)
        dense = resample(g, T, t)
        last = float(np.sqrt(t(d2)))
        its += 1
        if last < conv_tol:
            break
    return dict(T=T, dense=dense, iterations=its, last_delta_norm=last, ncorr=ncorr, warped=transform_points(dense, src))
