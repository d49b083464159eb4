"""Exact fixtures and an integer restatement for the 48 raw f64 sums of one ICP iteration (csrc/solve.hpp: SUMS_KABSCH / SUMS_PLANE /
SUMS_GN_FULL) -- what every accumulating kernel must produce BIT FOR BIT, whatever its order of additions, wave layout or block count.

Why the sums are exact here.  Every per-pair term is formed by individually rounded f32 operations (search_device.hpp: fused_z,
accumulate_pair), the products and sums in f64.  On this data every one of those operations is exact:
  * target points on an integer lattice of spacing 1 (origin (2, s + 3, 2 s + 4) for a cube of side s: the three coordinates of a point
    never coincide and none is 0 or 1), magnitudes below 2^8;
  * the transformed source q = lattice site + offset, offsets multiples of 2^-4 with |component| <= 3/16: the nearest target of a query
    is its own site at d2 = |offset|^2 <= 27/256, every other site is at least (13/16)^2 away -- unique by far more than one quantum;
  * target normals with components from +-{0.5, 1, 1.5, 2}, all three non-zero, NOT normalised: nothing between cilhip_set_target and the
    kernels normalises them (c_api.hip uploads, grid_build.hip's k_gather copies the three floats into the sorted float4, the kernels
    read z[3..5] = nv raw), so the issue's fall-back to the six signed axes was not needed.  Of the 512 such triples the fixture uses
    those whose six products n_i n_j are pairwise distinct and none of them 1 (a single pair's slots are then distinct);
  * means handed to the library (cilhip_set_shard_info / icp_begin's global_src_mean) in multiples of 1/4 -- they need not be the
    clouds' true means: the estimators only need the SAME numbers on both sides;
  * transforms from tests/_filter_refs.py's exact family (identity, a signed axis permutation with an integer shift, a mirror): the
    source handed over is T^-1 q, and the pinned expression (L0 x + (L1 y + L2 z)) + t gives q again bit for bit.
So every entry of the per-pair vector z is a multiple of 2^-5 below 2^11, every product a multiple of 2^-10, and each of the 48 sums ONE
exact number: `expected_sums` forms it as z^T W z in int64 (numerators over 2^13: per-pair weights are multiples of 2^-3) and
`assert_exact_fixture` shows that the f32 and the f64 evaluation of the term expressions agree and that nothing leaves 53 bits.

Distances.  A query's offset (a, b, c) / 16 has d2 = (a^2 + b^2 + c^2) / 256.  Ordinary queries get a^2 + b^2 + c^2 in 10 .. 22, the
query `lone` (index 0) one of the 56 offsets with three non-zero components and 3 .. 9, the query `far` (index n - 1, n >= 2) (+-3, +-3, +-3): 27.  `radius_between`
puts a squared radius halfway between two consecutive values (exactly representable; the engine's comparison d2 < max_sq is strict
either way), `masks` names the patterns: all, none, about half, all but one (`far` cut), exactly one (`lone` alone).  `with_lone`
makes any query k the lone one without touching the target.

Slots that are equal by definition: with unit weights slot 43 (sum of the point-term weights) IS slot 0 (the count); the distinctness
condition leaves that one pair out and holds every other pair of used slots apart."""
import numpy as np

import _filter_refs as fr

KABSCH, PLANE, POINT, BOTH = "kabsch", "plane", "point", "both"
METRICS = (KABSCH, PLANE, POINT, BOTH)
NSLOTS = 48
ZSCALE = 32              # every entry of z is a multiple of 2^-5
WSCALE = 8               # every per-pair weight (metric weight x pair weight) a multiple of 2^-3
DEN_LOG2 = 13            # numerators are over 2^13 = ZSCALE^2 * WSCALE
QUANTUM = 1.0 / 16.0

TRANSFORMS = ("identity", "rz90_shift", "mirror_z")      # of fr.TRANSFORMS

_TRIPLES = np.array([(a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)], np.int64)
_SS = (_TRIPLES ** 2).sum(1)
OFF_ORDINARY = _TRIPLES[(_SS >= 10) & (_SS <= 22)]
OFF_LONE = _TRIPLES[(_SS <= 9) & np.all(_TRIPLES != 0, 1)]      # (no component 0: a single pair's q differs from p along every axis)
OFF_FAR = _TRIPLES[_SS == 27]


def _normal_table():
    vals = [s * m for s in (-1.0, 1.0) for m in (0.5, 1.0, 1.5, 2.0)]
    out = []
    for a in vals:
        for b in vals:
            for c in vals:
                pr = [a * a, a * b, a * c, b * b, b * c, c * c]
                if len(set(pr)) == 6 and 1.0 not in pr:
                    out.append((a, b, c))
    return np.array(out, np.float32)


NORMALS = _normal_table()


def cube_side(n):
    s = max(1, int(round(n ** (1.0 / 3.0))))
    while s ** 3 < n:
        s += 1
    while s > 1 and (s - 1) ** 3 >= n:
        s -= 1
    return s


def lattice_sites(n, side):
    """the first n sites of the integer lattice inside a cube of `side`, x slowest; origin (2, side + 3, 2 side + 4)"""
    g = np.arange(n, dtype=np.int64)
    ijk = np.stack([g // (side * side), (g // side) % side, g % side], 1)
    return ijk + np.array([2, side + 3, 2 * side + 4], np.int64)


def _exact32(x64):
    x = np.ascontiguousarray(x64, np.float32)
    assert np.array_equal(x.astype(np.float64), x64)
    return x


def _stored(q64, tname):
    """s with T s == q exactly (fr.stored_source on f64 input)"""
    T, Linv = fr.TRANSFORMS[tname]
    return _exact32((q64 - T[:3, 3].astype(np.float64)) @ Linv.T)


def _stored_vectors(v64, tname):
    """n with T.linear() n == v exactly"""
    _T, Linv = fr.TRANSFORMS[tname]
    return _exact32(v64 @ Linv.T)


def lattice_pair(n, T="identity", kind="plain", n_target=None, seed=0):
    """-> dict: D, N (target points, normals), S (source as stored: T^-1 q), q (T S), T (4x4 f32), dst_mean, src_mean (dyadic; T src_mean =
    `smt` is dyadic too), match (target index of every source point's nearest target), off (integer offsets in 1/16), d2 (exact f32
    squared distances), lone / far, kind "symmetric": + SN (source normals as stored) and SNq (T.linear() SN, multiples of 1/2 up to 4).
    n_target (default: the whole cube that holds n sites) >= n: the target is a superset of the sites the source sits on."""
    assert kind in ("plain", "symmetric") and n >= 1
    rng = np.random.default_rng(1000 + seed)
    side = cube_side(n if n_target is None else max(n, n_target))
    nd = side ** 3 if n_target is None else int(n_target)
    assert nd >= n
    sites = lattice_sites(nd, side)
    perm_t = rng.permutation(nd)                       # target index of site j: index order is not grid order
    D64 = np.empty((nd, 3), np.float64)
    D64[perm_t] = sites
    N = NORMALS[rng.integers(0, len(NORMALS), nd)]
    site_of = rng.permutation(nd)[:n]                  # the site source point k sits on
    off = OFF_ORDINARY[rng.integers(0, len(OFF_ORDINARY), n)].copy()
    lone, far = 0, (n - 1 if n >= 2 else None)
    if far is not None:
        off[far] = OFF_FAR[rng.integers(0, len(OFF_FAR))]
    c = (side - 1) // 2
    dst_mean = np.array([2 + c + 0.25, side + 3 + c - 0.25, 2 * side + 4 + c + 0.5], np.float64)
    smt = np.array([2 + c - 0.25, side + 3 + c + 0.5, 2 * side + 4 + c + 0.25], np.float64)
    Tm, Linv = fr.TRANSFORMS[T]
    fix = {"name": f"lattice_{n}_{T}_{kind}", "n": n, "nd": nd, "side": side, "tname": T, "T": Tm.copy(), "D": _exact32(D64), "N": np.ascontiguousarray(N),
           "match": perm_t[site_of], "off": off, "lone": lone, "far": far, "dst_mean": _exact32(dst_mean), "smt": _exact32(smt),
           "src_mean": _exact32((smt - Tm[:3, 3].astype(np.float64)) @ Linv.T), "kind": kind}
    if kind == "symmetric":
        # (the vector the terms see, n_dst + T.linear() n_src, is again one of NORMALS; no component of the source normal is 0)
        nd_k = N[fix["match"]].astype(np.float64)
        SNq = np.zeros((n, 3))
        while True:
            bad = np.nonzero(np.any(SNq == 0.0, 1))[0]
            if len(bad) == 0:
                break
            SNq[bad] = NORMALS[rng.integers(0, len(NORMALS), len(bad))].astype(np.float64) - nd_k[bad]
        fix["SNq"] = _exact32(SNq)
        fix["SN"] = _stored_vectors(SNq, T)
    _place(fix)
    return with_lone(fix, lone, _copy=False)


def _place(fix):
    q64 = fix["D"].astype(np.float64)[fix["match"]] + fix["off"] * QUANTUM
    fix["q"] = _exact32(q64)
    fix["S"] = _stored(q64, fix["tname"])
    fix["d2"] = _exact32((fix["off"] ** 2).sum(1) / 256.0)


def with_lone(fix, k, _copy=True):
    """the fixture with query k as the only one below d2 = 10/256: the former lone query gets an ordinary offset, k one of the 56 small
    ones -- the first (in a seeded order) under which the single pair's used slots are non-zero and pairwise distinct in all four metrics"""
    out = dict(fix) if _copy else fix
    out.pop("_checked", None)
    off = fix["off"].copy()
    rng = np.random.default_rng(7 + 31 * k + fix["n"])
    old = fix["lone"]
    if old != k:
        off[old] = OFF_ORDINARY[rng.integers(0, len(OFF_ORDINARY))]
    out["lone"] = k
    if fix["far"] == k:                                 # (n >= 2: another query takes the far place)
        out["far"] = old
        off[old] = OFF_FAR[rng.integers(0, len(OFF_FAR))]
    has = np.zeros(fix["n"], bool)
    has[k] = True
    for cand in OFF_LONE[rng.permutation(len(OFF_LONE))]:
        off[k] = cand
        out["off"] = off
        _place(out)
        if all(_distinct_nonzero(m, expected_sums_of(out, m, has)[0]) for m in METRICS):
            return out
    raise AssertionError(("no offset keeps the single pair's slots apart", fix["name"], k))


# ---- the term expressions, evaluated step by step in one dtype (numpy rounds every operation on its own: no contraction) ---------------

def transform_points(T, S, dt):
    """the pinned expression (L0 x + (L1 y + L2 z)) + t"""
    L = np.asarray(T, np.float32)[:3, :3].astype(dt); t = np.asarray(T, np.float32)[:3, 3].astype(dt)
    S = np.asarray(S).astype(dt).reshape(-1, 3)
    return np.stack([(L[r, 0] * S[:, 0] + (L[r, 1] * S[:, 1] + L[r, 2] * S[:, 2])) + t[r] for r in range(3)], 1)


def rotate_vectors(T, V, dt):
    """T.linear() v in the x + (y + z) pairing of accumulate_pair's sym branch (the inner linear part that follows is the identity on the
    first Gauss-Newton step: 1 * t_r plus zeros)"""
    L = np.asarray(T, np.float32)[:3, :3].astype(dt)
    V = np.asarray(V).astype(dt).reshape(-1, 3)
    return np.stack([L[r, 0] * V[:, 0] + (L[r, 1] * V[:, 1] + L[r, 2] * V[:, 2]) for r in range(3)], 1)


def pair_terms(metric, p, nv, q, dst_mean, smt, dt, sn_rot=None):
    """z per pair (rows), as fused_z / accumulate_pair form it on the first Gauss-Newton step (inner transform = identity):
    KABSCH (p, q, 1); PLANE (e0..e5, res, 1); POINT (a, r, 1); BOTH (e0..e5, res, 1, a, r).  sn_rot: the symmetric objective's
    T.linear() n_src, added to the target normal"""
    p = np.asarray(p).astype(dt); q = np.asarray(q).astype(dt)
    one = np.ones((len(p), 1), dt)
    if metric == KABSCH:
        return np.concatenate([p, q, one], 1)
    d = p - np.asarray(dst_mean).astype(dt)[None, :]
    s = q - np.asarray(smt).astype(dt)[None, :]
    a = d + s
    r = d - s
    if metric == POINT:
        return np.concatenate([a, r, one], 1)
    n = np.asarray(nv).astype(dt)
    if sn_rot is not None:
        n = n + np.asarray(sn_rot).astype(dt)
    e = np.stack([a[:, 1] * n[:, 2] - a[:, 2] * n[:, 1], a[:, 2] * n[:, 0] - a[:, 0] * n[:, 2], a[:, 0] * n[:, 1] - a[:, 1] * n[:, 0]], 1)
    res = (n[:, 0] * r[:, 0] + (n[:, 1] * r[:, 1] + n[:, 2] * r[:, 2]))[:, None]
    z = np.concatenate([e, n, res, one], 1)
    return z if metric == PLANE else np.concatenate([z, a, r], 1)


def _int_rows(z64, scale):
    zi = np.rint(z64 * scale).astype(np.int64)
    assert np.array_equal(zi.astype(np.float64) / scale, z64), "an entry is not a multiple of 1 / %d" % scale
    return zi


def _tri(k):
    return [(r, c) for r in range(k) for c in range(r, k)]


def used_slots(metric):
    if metric == KABSCH:
        return list(range(16))
    if metric == PLANE:
        return list(range(28))
    if metric == POINT:
        return [0] + list(range(28, 44))
    return list(range(44))


def slot_numerators(metric, M_one, M_pl, M_pt, sum_wq):
    """the 48 slots (solve.hpp:20-29) from z^T W z: M_one with unit weights (x WSCALE), M_pl with the plane weights, M_pt with the
    point weights, all as Python-int matrices over 2^13"""
    out = [0] * NSLOTS
    if metric == KABSCH:
        one = 6
        out[0] = M_one[one][one]
        for c in range(3):
            out[1 + c] = M_one[c][one]
            out[4 + c] = M_one[3 + c][one]
        for r in range(3):
            for c in range(3):
                out[7 + 3 * r + c] = M_one[r][3 + c]
        return out
    one = 6 if metric == POINT else 7
    out[0] = M_one[one][one]
    if metric in (PLANE, BOTH):
        for k, (r, c) in enumerate(_tri(6)):
            out[1 + k] = M_pl[r][c]
        for r in range(6):
            out[22 + r] = M_pl[6][r]
    if metric in (POINT, BOTH):
        A, R = (0, 3) if metric == POINT else (8, 11)
        for c in range(3):
            out[28 + c] = M_pt[A + c][one]
            out[40 + c] = M_pt[R + c][one]
        for k, (r, c) in enumerate(_tri(3)):
            out[31 + k] = M_pt[A + r][A + c]
        out[37] = M_pt[A + 1][R + 2] - M_pt[A + 2][R + 1]
        out[38] = M_pt[A + 2][R + 0] - M_pt[A + 0][R + 2]
        out[39] = M_pt[A + 0][R + 1] - M_pt[A + 1][R + 0]
        out[43] = sum_wq
    return out


def _gram(zi, w, force_int=False):
    """z^T diag(w) z as Python ints.  Up to 4096 rows in int64; beyond, an f64 matrix product (BLAS) -- exact whatever its order of
    additions, because the sum of the absolute values of any entry's terms stays below 2^53 (asserted)"""
    if len(zi) <= 4096 or force_int:
        return ((zi * w[:, None]).T @ zi).tolist()      # |z| < 2^16, w <= 2^5, 2^20 pairs stay below 2^62
    zf = zi.astype(np.float64)
    col = np.abs(zf).max(0)
    assert float(np.outer(col, col).max()) * float(w.max()) * len(zi) < 2.0 ** 53
    return [[int(v) for v in row] for row in (zf * w.astype(np.float64)[:, None]).T @ zf]


def expected_sums(metric, D, N, S, T, dst_mean, src_mean, match, has, weights=None, src_normals=None):
    """-> (numerators: 48 Python ints over 2^DEN_LOG2, their f64 image).  match[k]: target index of source point k; has[k]: the pair
    counts; weights: (wq, wp) per source point (the products metric weight x pair weight, multiples of 1/8) or None = unit;
    src_normals: the symmetric objective's source normals as stored"""
    has = np.asarray(has, bool)
    idx = np.nonzero(has)[0]
    q = transform_points(T, np.asarray(S)[idx], np.float64)
    smt = transform_points(T, np.asarray(src_mean).reshape(1, 3), np.float64)[0]
    sn = None if src_normals is None or metric in (KABSCH, POINT) else rotate_vectors(T, np.asarray(src_normals)[idx], np.float64)
    mi = np.asarray(match)[idx]
    z = pair_terms(metric, np.asarray(D)[mi], None if N is None else np.asarray(N)[mi], q, dst_mean, smt, np.float64, sn)
    zi = _int_rows(z, ZSCALE)
    unit = np.full(len(idx), WSCALE, np.int64)
    if weights is None:
        wq = wp = unit
    else:
        wq = _int_rows(np.asarray(weights[0], np.float64)[idx], WSCALE)
        wp = _int_rows(np.asarray(weights[1], np.float64)[idx], WSCALE)
    M_one = _gram(zi, unit)
    M_pl = M_one if weights is None else _gram(zi, wp)
    M_pt = M_one if weights is None else _gram(zi, wq)
    num = slot_numerators(metric, M_one, M_pl, M_pt, int(wq.sum()) * ZSCALE * ZSCALE)
    return num, np.array([v / float(1 << DEN_LOG2) for v in num], np.float64)


def expected_sums_of(fix, metric, has, weights=None):
    return expected_sums(metric, fix["D"], fix["N"], fix["S"], fix["T"], fix["dst_mean"], fix["src_mean"], fix["match"], has, weights,
                         fix.get("SN"))


def _distinct_nonzero(metric, num):
    v = [num[s] for s in used_slots(metric) if not (s == 43)]       # (slot 43 is slot 0 by definition)
    return all(x != 0 for x in v) and len(set(v)) == len(v)


def gn_normal_equations(sums, w_p2p, w_p2pl, point_weighted=False):
    """solve.hpp's gn_normal_equations restated -> (AtA 6x6, Atb 6): on exact sums with dyadic weights every operation is exact"""
    s = np.asarray(sums, np.float64)
    AtA = np.zeros((6, 6)); Atb = np.zeros(6)
    if w_p2pl > 0.0:
        for k, (a, b) in enumerate(_tri(6)):
            v = w_p2pl * s[1 + k]
            AtA[a, b] += v
            if a != b:
                AtA[b, a] += v
        Atb += w_p2pl * s[22:28]
    if w_p2p > 0.0:
        n = s[43] if point_weighted else s[0]
        sa = s[28:31]
        aa = np.zeros((3, 3))
        for k, (r, c) in enumerate(_tri(3)):
            aa[r, c] = aa[c, r] = s[31 + k]
        X = np.array([[0.0, -sa[2], sa[1]], [sa[2], 0.0, -sa[0]], [-sa[1], sa[0], 0.0]])
        AtA[:3, :3] += w_p2p * (np.trace(aa) * np.eye(3) - aa)
        AtA[:3, 3:] += w_p2p * X
        AtA[3:, :3] += w_p2p * X.T
        AtA[3:, 3:] += w_p2p * n * np.eye(3)
        Atb[:3] += w_p2p * s[37:40]
        Atb[3:] += w_p2p * s[40:43]
    return AtA, Atb


# ---- the affine classes' normal equations (solve.hpp:515-519; the IM_AFF0 / 1 / 2 passes of internal.hpp:101-108 feed them) -----------------

def affine_terms(p, nv, q, dst_mean, smt, dt):
    """per pair: st = (s, 1), d, u[(j, a)] = n_j st_a, res = n . d, in one dtype; s = q - T src_mean, d = p - dst_mean (both means zero for
    the point-to-point class), index (j, a) = 3 j + a for a < 3, 9 + j for the translation"""
    p = np.asarray(p).astype(dt); q = np.asarray(q).astype(dt); n = np.asarray(nv).astype(dt)
    d = p - np.asarray(dst_mean).astype(dt)[None, :]
    s = q - np.asarray(smt).astype(dt)[None, :]
    st = np.concatenate([s, np.ones((len(p), 1), dt)], 1)
    res = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
    return st, d, n, res


def _aff_idx(j, a):
    return 3 * j + a if a < 3 else 9 + j


def expected_affine(fix, has, w_pt, w_pl, centered):
    """-> (AtA 12x12, Atb 12, count) of cilhip_estimate_affine: AtA[(j,a),(k,b)] = w_pl sum n_j n_k st_a st_b + w_pt delta_jk sum st_a st_b,
    Atb[(j,a)] = w_pl sum (n.d) n_j st_a + w_pt sum st_a d_j.  Every product is a multiple of 2^-10 and every sum of absolute values stays
    below 2^53 (asserted), so the f64 matrix products are exact"""
    idx = np.nonzero(np.asarray(has, bool))[0]
    zero = np.zeros(3, np.float32)
    dm, smt = (fix["dst_mean"], fix["smt"]) if centered else (zero, zero)
    mi = fix["match"][idx]
    st, d, n, res = affine_terms(fix["D"][mi], fix["N"][mi], fix["q"][idx], dm, smt, np.float64)
    u = np.zeros((len(idx), 12))
    for j in range(3):
        for a in range(4):
            u[:, _aff_idx(j, a)] = n[:, j] * st[:, a]
    bound = len(idx) * max(1.0, float(np.abs(u).max(initial=0)) ** 2, float(np.abs(res).max(initial=0) * np.abs(u).max(initial=0)),
                           float(np.abs(st).max(initial=0)) ** 2, float(np.abs(st).max(initial=0) * np.abs(d).max(initial=0))) * 2.0 ** 10
    assert bound < 2.0 ** 53
    AtA = np.zeros((12, 12)); Atb = np.zeros(12)
    if w_pl > 0.0:
        AtA += w_pl * (u.T @ u)
        Atb += w_pl * (res @ u)
    if w_pt > 0.0:
        SS = st.T @ st
        Sd = st.T @ d
        for j in range(3):
            for a in range(4):
                for b in range(4):
                    AtA[_aff_idx(j, a), _aff_idx(j, b)] += w_pt * SS[a, b]
                Atb[_aff_idx(j, a)] += w_pt * Sd[a, j]
    return AtA, Atb, len(idx)


def assert_exact_affine(fix, centered):
    zero = np.zeros(3, np.float32)
    dm, smt = (fix["dst_mean"], fix["smt"]) if centered else (zero, zero)
    p, nv = fix["D"][fix["match"]], fix["N"][fix["match"]]
    t32 = affine_terms(p, nv, fix["q"], dm, smt, np.float32)
    t64 = affine_terms(p, nv, fix["q"], dm, smt, np.float64)
    for a, b in zip(t32, t64):
        assert a.dtype == np.float32 and np.array_equal(a.astype(np.float64), b), fix["name"]


# ---- radius masks ----------------------------------------------------------------------------------------------------------------------

def radius_between(d2_values, k):
    """a squared radius halfway between the k-th and the (k+1)-th distinct value of d2_values (ascending; k = 0: half the smallest,
    k = their number: the largest plus half the smallest): exactly k distinct values lie below it, none on it"""
    v = np.unique(np.asarray(d2_values, np.float64))
    assert len(v) and v[0] > 0.0 and 0 <= k <= len(v)
    r = 0.5 * v[0] if k == 0 else (v[-1] + 0.5 * v[0] if k == len(v) else 0.5 * (v[k - 1] + v[k]))
    r32 = np.float32(r)
    assert float(r32) == r and not np.any(v == r)
    return r32


def masks(fix):
    """name -> (squared radius, has): all, none, half, all_but_one, one -- those that exist at this size and differ from one another"""
    d2 = fix["d2"].astype(np.float64)
    v = np.unique(d2)
    out, seen = {}, set()
    below = [int((d2 < x).sum()) for x in v] + [len(d2)]      # queries below a radius that keeps k distinct values
    k_half = min(range(len(v) + 1), key=lambda k: abs(below[k] - len(d2) / 2.0))
    for name, k in (("all", len(v)), ("none", 0), ("half", k_half), ("all_but_one", len(v) - 1), ("one", 1)):
        r = radius_between(d2, k)
        has = d2 < float(r)
        cnt = int(has.sum())
        want = {"all": len(d2), "none": 0, "all_but_one": len(d2) - 1, "one": 1}.get(name)
        if (want is not None and cnt != want) or cnt in seen:
            continue
        seen.add(cnt)
        out[name] = (r, has)
    return out


# ---- the conditions that make an exact comparison meaningful ---------------------------------------------------------------------------

def assert_exact_fixture(fix, metric, has, weights=None, brute=False):
    """(1) every f32 operation of the term expressions is exact: the f32 and the f64 evaluation agree, for the transformed source, the
    transformed mean, the distances and z; (2) every slot's numerator stays below 2^53; (3) with at least one pair, the metric's used
    slots are non-zero and pairwise distinct (slot 43 aside: it is slot 0), so no swap can hide; (4) every query's nearest target is
    unique by at least one offset quantum (by construction: its own site; brute = True also searches, for the small sizes)."""
    key = (metric, fix["lone"], None if weights is None else "w")
    if key not in fix.setdefault("_checked", set()) or brute:
        _assert_exact_terms(fix, metric, weights, brute)
        fix["_checked"].add(key)
    num, f64 = expected_sums_of(fix, metric, has, weights)
    assert all(abs(v) < (1 << 53) for v in num), (fix["name"], metric)
    assert [int(v * (1 << DEN_LOG2)) for v in f64] == num
    if np.any(has) and weights is None:
        assert _distinct_nonzero(metric, num), (fix["name"], metric, int(np.sum(has)))
    assert all(num[s] == 0 for s in range(NSLOTS) if s not in used_slots(metric))
    return num, f64


def _assert_exact_terms(fix, metric, weights, brute):
    """conditions (1) and (4) of assert_exact_fixture: they do not depend on the mask"""
    n = fix["n"]
    T = fix["T"]
    q32 = transform_points(T, fix["S"], np.float32); q64 = transform_points(T, fix["S"], np.float64)
    assert np.array_equal(q32.astype(np.float64), q64) and np.array_equal(q32, fix["q"]), fix["name"]
    m32 = transform_points(T, fix["src_mean"].reshape(1, 3), np.float32)[0]
    assert np.array_equal(m32, fix["smt"]) and np.array_equal(m32.astype(np.float64), transform_points(T, fix["src_mean"].reshape(1, 3), np.float64)[0])
    p = fix["D"][fix["match"]]
    df = q32 - p
    d2_32 = df[:, 0] * df[:, 0] + (df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2])
    assert np.array_equal(d2_32, fix["d2"]) and np.array_equal(d2_32.astype(np.float64), ((q64 - p.astype(np.float64)) ** 2).sum(1))
    sn32 = sn64 = None
    if "SN" in fix and metric in (PLANE, BOTH):
        sn32 = rotate_vectors(T, fix["SN"], np.float32); sn64 = rotate_vectors(T, fix["SN"], np.float64)
        assert np.array_equal(sn32.astype(np.float64), sn64) and np.array_equal(sn32, fix["SNq"])
    z32 = pair_terms(metric, p, fix["N"][fix["match"]], q32, fix["dst_mean"], m32, np.float32, sn32)
    z64 = pair_terms(metric, p, fix["N"][fix["match"]], q64, fix["dst_mean"], m32, np.float64, sn64)
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64), (fix["name"], metric)
    if weights is not None:
        for w in weights:                                # __fmul_rn(w, e): a dyadic weight times a 16-bit entry
            w32 = np.asarray(w, np.float32)
            assert np.array_equal((w32[:, None] * z32).astype(np.float64), w32.astype(np.float64)[:, None] * z64)
    # (4) the nearest site of q is the designated one, the offsets are within 3/16: any other lattice site is >= 13/16 away along an axis
    assert np.abs(fix["off"]).max() <= 3 and np.array_equal(np.rint(q64), p.astype(np.float64))
    assert len(np.unique(fix["match"])) == n
    assert float(fix["d2"].max()) + QUANTUM <= (1.0 - 3 * QUANTUM) ** 2
    if brute:
        D64 = fix["D"].astype(np.float64)
        for k in range(n):
            dd = ((D64 - q64[k]) ** 2).sum(1)
            o = np.argsort(dd)
            assert o[0] == fix["match"][k] and (len(o) == 1 or dd[o[1]] - dd[o[0]] >= QUANTUM), (fix["name"], k)


# ---- the case table both test modules walk ---------------------------------------------------------------------------------------------

SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 65536, 65537, 65599, 524288, 524289)
WARM_SIZES = tuple(n for n in SIZES if n >= 65536)      # warm_capable(): ns >= 65536
SINGLE_SIZES = (64, 65, 257)                            # every query in turn as the only match
STORED_SIZES = (1, 65, 257, 2049, 524289)               # the host entries over a stored set
LOOP_SIZES = (257, 2049, 65537)                         # one iteration of the device-resident loops
A_TRANSFORMS = ("identity", "rz90_shift")
DYADIC_WEIGHTINGS = ((0.0, 1.0), (1.0, 0.0), (0.5, 0.25))      # (w_p2p, w_p2pl)
PAIR_WEIGHT_VALUES = (0.0, 0.5, 1.0, 2.0)

_cache = {}
_seed = {}


def fixture(n, T="identity", kind="plain"):
    """the case table's fixture: seed 0, or -- below 4096 points, where two or three pairs can make two slots meet by chance -- the first seed
    whose masks keep every metric's used slots non-zero and apart (the same seed for every transform: one target serves them all)"""
    key = (n, T, kind)
    if key not in _cache:
        seed = _seed.get((n, kind))
        if seed is None:
            seed = 0
            while n < 4096 and not _masks_distinct(lattice_pair(n, "identity", kind, seed=seed)):
                seed += 1
            _seed[(n, kind)] = seed
        _cache[key] = lattice_pair(n, T, kind, seed=seed)
    return _cache[key]


def single_match_fixture(n, k):
    """the single-match case k of size n: query k the lone one, even k under the identity, odd k under the quarter turn"""
    return with_lone(fixture(n, A_TRANSFORMS[k % 2]), k)


def _masks_distinct(fix):
    return all(_distinct_nonzero(m, expected_sums_of(fix, m, has)[0]) for _r, has in masks(fix).values() if has.any() for m in METRICS)


def metric_of_weights(w_p2p, w_p2pl):
    return BOTH if (w_p2p > 0 and w_p2pl > 0) else (PLANE if w_p2pl > 0 else POINT)


def pair_weights(fix, has, seed=3):
    """dyadic per-pair weights (point, plane) from PAIR_WEIGHT_VALUES, per source point; a zero sits inside an otherwise full wave: the
    first matched query gets (0, 0), the second (0, 2), the third (2, 0)"""
    rng = np.random.default_rng(seed + fix["n"])
    v = np.array(PAIR_WEIGHT_VALUES, np.float32)
    wq = v[rng.integers(0, 4, fix["n"])]; wp = v[rng.integers(0, 4, fix["n"])]
    idx = np.nonzero(has)[0]
    for k, (a, b) in zip(idx[:3], ((0.0, 0.0), (0.0, 2.0), (2.0, 0.0))):
        wq[k], wp[k] = a, b
    return wq, wp


# ---- two exact iterations: a fixture whose FIRST STEP is exact (section D of tests/test_gpu_exact_sums.py) -------------------------------
#
# The second iteration of a run sees lattice data again if the first one steps onto an exactly representable transform.  Target: the
# integer lattice as above (origin (6, side + 10, 2 side + 14): under the quarter turn with its shift no stored source coordinate
# comes near zero), normals from NORMALS, plus TWIN target points beside some occupied sites.  Source, by group (offsets in 1/16):
#   A  site + U            matched in both iterations; every centred residual of iteration 0 is the same vector, so x* = (0, 0, 0, t)
#                          solves every pair's equation in all four metrics, Kabsch's sigma = cov(p, p) has the identity as its polar
#                          factor, and the step is the translation by -U / 16: T1 = T0 with that translation, to round-off in the
#                          linear part (ABSORB says how much of it the pinned transform expression swallows)
#   B  site + U + delta    |U + delta|^2 >= 11: unmatched at iteration 0; |delta|^2 <= 10: matched at iteration 1 with residual
#                          -delta / 16, so Atb != 0 and T2 depends on every slot
#   F  site + F            never matched (|F|^2 >= 11 and |F - U|^2 >= 11); sites without a source point besides (nd > n)
#   twin targets           site + W beside some A sites, |W - U|^2 >= 11 and 0 < |W|^2 <= 10: unmatched at iteration 0; at iteration 1
#                          their nearest source point is the A point ON the site, whose own nearest target is the site: a reverse
#                          match that is no reciprocal duplicate (mode 2 counts it, mode 3 does not)
# squared radius between 10/256 and 11/256.  Expected sets: iteration 0, every direction: the A pairs; iteration 1: FIRST_TO_SECOND
# A + B + twins; BOTH the forward A + B plus the reverse non-duplicates = the twins; BOTH reciprocal A + B.

TWO_STEP_U = np.array((1, 1, 1), np.int64)
TWO_STEP_DELTAS = np.array(((2, 1, 1), (2, 2, 1), (2, 2, 0), (2, 0, 2)), np.int64)
TWO_STEP_F = np.array((-3, -3, -3), np.int64)
TWO_STEP_W = np.array((-2, -1, -1), np.int64)
TWO_STEP_LARGE = 16 * 2048 * 256 + 257        # reverse_warm_blocks() capped at 2048 blocks, 17 rounds in the first of them
TWO_STEP_SIZES = (255, 256, 257, 2048, 2049, 4097 + 255, TWO_STEP_LARGE)      # target points, twins included
TWO_STEP_DIRECTIONS = ("first_to_second", "both", "both_reciprocal")
GROUP_A, GROUP_B, GROUP_F = 0, 1, 2
# a perturbation of every entry of T1's linear part that transform_points must still round away: the smallest stored coordinate is above
# 2 (half an ulp: 2^-23), the sum of a point's coordinates below 2^11, so anything below 2^-34 disappears; the solves leave ~1e-15
ABSORB = 2.0 ** -36

_two_step_targets = {}
_two_step_cache = {}


def _two_step_target(nd, seed):
    """the target of size nd (shared by every T0): sites, twins beside the first n_tw A sites, the source's groups and sites"""
    key = (nd, seed)
    if key in _two_step_targets:
        return _two_step_targets[key]
    rng = np.random.default_rng(5000 + seed)
    n_tw = min(max(8, nd // 32), 256)
    n_sites = nd - n_tw
    side = cube_side(n_sites)
    origin = np.array([6, side + 10, 2 * side + 14], np.int64)
    n = min(int(0.55 * n_sites), 4096)
    n_a = int(0.6 * n)
    n_b = int(0.3 * n)
    assert n_a >= 16 and n_a >= n_tw and n_b >= len(TWO_STEP_DELTAS) and n - n_a - n_b >= 1
    # the source sits in the low corner of the lattice (all of it below 2^16 sites): small coordinates whatever the target's size
    sub = side if n_sites <= 65536 else 24
    g = np.arange(min(n_sites, (sub - 1) * (side * side + side + 1) + 1), dtype=np.int64)
    ijk = np.stack([g // (side * side), (g // side) % side, g % side], 1)
    cand = g[np.all(ijk < sub, 1)]
    site_g = rng.choice(cand, n, replace=False)                          # lattice index of the site source point k sits on
    group = np.full(n, GROUP_F, np.int64)
    group[:n_a] = GROUP_A
    group[n_a:n_a + n_b] = GROUP_B
    group = group[rng.permutation(n)]
    a_idx = np.nonzero(group == GROUP_A)[0]
    tw_s = a_idx[rng.permutation(len(a_idx))[:n_tw]]                     # the A point on every twin's site
    gs = np.arange(n_sites, dtype=np.int64)
    sites = np.stack([gs // (side * side), (gs // side) % side, gs % side], 1) + origin
    D64 = np.empty((nd, 3), np.float64)
    perm_t = rng.permutation(nd)                                         # target index of (site j | twin j - n_sites)
    D64[perm_t[:n_sites]] = sites
    D64[perm_t[n_sites:]] = sites[site_g[tw_s]] + TWO_STEP_W * QUANTUM
    N = NORMALS[rng.integers(0, len(NORMALS), nd)]
    off = np.empty((n, 3), np.int64)
    off[group == GROUP_A] = TWO_STEP_U
    nb = int((group == GROUP_B).sum())
    off[group == GROUP_B] = TWO_STEP_U + TWO_STEP_DELTAS[np.arange(nb) % len(TWO_STEP_DELTAS)]
    off[group == GROUP_F] = TWO_STEP_F
    c = sites[site_g].mean(0).astype(np.int64)
    tgt = {"nd": nd, "n": n, "n_sites": n_sites, "side": side, "D": _exact32(D64), "N": np.ascontiguousarray(N), "group": group, "off": off,
           "site_t": perm_t[site_g], "tw_t": perm_t[n_sites:], "tw_s": tw_s,
           "dst_mean": _exact32(c + np.array([0.25, -0.25, 0.5])), "smt0": _exact32(c + np.array([-0.25, 0.5, 0.25])),
           "r2": radius_between(np.array([10.0, 11.0]) / 256.0, 1)}
    _two_step_targets[key] = tgt
    return tgt


def two_step_pair(nd, T="identity", seed=0):
    """-> dict: D, N, S, T (= T0), T1 (T0 moved by -U/16: where iteration 0 must step to), dst_mean, src_mean, smt0 / smt1 (T0 / T1 src_mean),
    q0 / q1 (the source under T0 / T1: q1 = q0 - U/16, on its site for A), r2, group, site_t (target index of every source point's site),
    tw_t / tw_s (twin targets and the A point on their site), pairs0 and pairs1[direction]: (target indices, source indices)"""
    key = (nd, T, seed)
    if key in _two_step_cache:
        return _two_step_cache[key]
    tgt = _two_step_target(nd, seed)
    Tm, Linv = fr.TRANSFORMS[T]
    fix = dict(tgt)
    q0 = tgt["D"].astype(np.float64)[tgt["site_t"]] + tgt["off"] * QUANTUM
    step = TWO_STEP_U * QUANTUM
    T1 = Tm.copy()
    T1[:3, 3] = _exact32(Tm[:3, 3].astype(np.float64) - step)
    fix.update({"name": f"two_step_{nd}_{T}", "tname": T, "T": Tm.copy(), "T1": T1, "q0": _exact32(q0), "q1": _exact32(q0 - step), "S": _stored(q0, T),
                "smt1": _exact32(tgt["smt0"].astype(np.float64) - step), "src_mean": _exact32((tgt["smt0"].astype(np.float64) - Tm[:3, 3].astype(np.float64)) @ Linv.T)})
    a = np.nonzero(tgt["group"] == GROUP_A)[0]
    ab = np.nonzero(tgt["group"] != GROUP_F)[0]
    fix["pairs0"] = (tgt["site_t"][a], a)
    with_twins = (np.concatenate([tgt["site_t"][ab], tgt["tw_t"]]), np.concatenate([ab, tgt["tw_s"]]))
    fix["pairs1"] = {"first_to_second": with_twins, "both": with_twins, "both_reciprocal": (tgt["site_t"][ab], ab)}
    _two_step_cache[key] = fix
    return fix


def expected_sums_pairs(fix, metric, T, pairs):
    """the exact sums over an explicit list of (target index, source index) pairs under T: a source point may occur in several pairs"""
    ti, si = pairs
    return expected_sums(metric, fix["D"], fix["N"], fix["S"][si], T, fix["dst_mean"], fix["src_mean"], ti, np.ones(len(ti), bool))


def _site_keys(x64):
    r = np.rint(x64).astype(np.int64)
    return (r[:, 0] * 4096 + r[:, 1]) * 4096 + r[:, 2]


def nearest_by_site(X, Y):
    """for every point of X its nearest point of Y, in f64 -> (index or -1, d2, d2 of the second nearest or inf).  Only points of Y whose
    rounded site lies in the 3 x 3 x 3 block around the rounded site of x are looked at: every point here is within 1/4 of its site, so
    any other point is more than 1 away and x is reported as having no neighbour (-1, inf) when the block is empty -- enough wherever the
    question is `inside a radius below 1/2`.  tests/test_sums_refs_cpu.py holds it against the full distance matrix at the small sizes."""
    X = np.asarray(X, np.float64); Y = np.asarray(Y, np.float64)
    ky = _site_keys(Y)
    oy = np.argsort(ky, kind="stable")
    kys = ky[oy]
    lo, hi = np.rint(Y.min(0)) - 1, np.rint(Y.max(0)) + 1
    near = np.nonzero(np.all((X >= lo - 0.5) & (X <= hi + 0.5), 1))[0]      # (the others' blocks hold no site of Y)
    idx = np.full(len(X), -1, np.int64); d1 = np.full(len(X), np.inf); d2 = np.full(len(X), np.inf)
    kx = _site_keys(X[near])
    bi = np.full(len(near), -1, np.int64); b1 = np.full(len(near), np.inf); b2 = np.full(len(near), np.inf)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = kx + (dx * 4096 + dy) * 4096 + dz
                beg = np.searchsorted(kys, k, "left"); end = np.searchsorted(kys, k, "right")
                for j in range(int((end - beg).max(initial=0))):
                    m = np.nonzero(beg + j < end)[0]
                    c = oy[beg[m] + j]
                    e = ((X[near[m]] - Y[c]) ** 2).sum(1)
                    better = e < b1[m]
                    b2[m] = np.where(better, b1[m], np.minimum(b2[m], e))
                    bi[m] = np.where(better, c, bi[m])
                    b1[m] = np.where(better, e, b1[m])
    idx[near] = bi; d1[near] = b1; d2[near] = b2
    return idx, d1, d2


def directed_sets(fix, q, r2):
    """-> (forward: (target, source) for every source point with a target inside the radius; reverse: the same for every target point),
    asserting that no nearest neighbour is tied and no distance is at the radius"""
    D64 = fix["D"].astype(np.float64); q64 = np.asarray(q, np.float64)
    out = []
    for X, Y in ((q64, D64), (D64, q64)):
        idx, d1, d2 = nearest_by_site(X, Y)
        has = d1 < float(r2)
        assert not np.any(d1 == float(r2)) and np.all(d2[has] - d1[has] >= 1.0 / 256.0), fix["name"]
        out.append((idx, has))
    (fi, fh), (ri, rh) = out
    s = np.nonzero(fh)[0]; t = np.nonzero(rh)[0]
    return (fi[s], s), (t, ri[t])


def _pair_set(pairs):
    return set(zip(np.asarray(pairs[0]).tolist(), np.asarray(pairs[1]).tolist()))


def loop_sets(fix, q, r2):
    """the correspondence set of each direction from the two searches: FIRST_TO_SECOND the reverse matches; BOTH their union with the
    forward ones; BOTH reciprocal the intersection -- as sets of (target, source)"""
    fwd, rev = directed_sets(fix, q, r2)
    f, r = _pair_set(fwd), _pair_set(rev)
    return {"first_to_second": r, "both": f | r, "both_reciprocal": f & r, "forward": f}


# ---- the grid the library lays over a cloud, restated (grid_policy.hpp: grid_first_cell, grid_set_dims; grid_build.hip: cell_of, a stable
# sort by cell key) -- where a target point sits in the order the reverse kernels walk; the GPU test holds the shape against get_grid_info

def grid_order(P, order=True):
    """-> dict: nx, ny, nz, cell, origin and, with `order`, occupancy and order (sorted position -> index into P)"""
    P = np.asarray(P, np.float32)
    lo, hi = P.min(0), P.max(0)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    maxext = float(ext.max())
    cell = float(np.cbrt(np.prod(np.maximum(ext, maxext * 1e-3)) / len(P)))
    cell = max(cell, maxext / 2047.0)
    f = np.float32
    while True:
        cf = f(cell); inv = f(1.0) / cf
        o = lo - f(2.0) * cf
        coord = lambda v, o_: np.floor(np.minimum(np.maximum((v - o_) * inv, f(-1.0)), f(1.0e9))).astype(np.int64)
        for c in range(3):
            if coord(lo[c], o[c]) < 2:
                o[c] = lo[c] - f(2.25) * cf
        dims = [max(int(np.floor(ext[c] / cell)) + 5, int(coord(hi[c], o[c])) + 3) for c in range(3)]
        if dims[0] * dims[1] * dims[2] <= 2 ** 26 and max(dims) <= 2048:
            break
        cell *= 1.1
    shape = {"nx": dims[0], "ny": dims[1], "nz": dims[2], "cell": float(cf), "origin": [float(v) for v in o]}
    if not order:
        return shape
    cc = [np.clip(coord(P[:, c], o[c]), 0, dims[c] - 1) for c in range(3)]
    key = (cc[2] * dims[1] + cc[1]) * dims[0] + cc[0]
    cnt = np.bincount(key).astype(np.float64)
    shape.update({"occupancy": float((cnt * cnt).sum() / len(P)), "order": np.argsort(key, kind="stable")})
    return shape


def reverse_walk_places(fix):
    """where the A sites' and the twin target points sit in the reverse kernels' walk over the sorted target (rounds of 256, waves of 64):
    -> dict of counts: in the last round, in lane 0 / lane 63 of a wave, for `a` and `twin`"""
    g = grid_order(fix["D"])
    assert g["occupancy"] <= 3.0      # (build_grid() keeps its first grid)
    pos = np.empty(fix["nd"], np.int64)
    pos[g["order"]] = np.arange(fix["nd"])
    last_round = (fix["nd"] - 1) // 256
    out = {}
    for name, t in (("a", fix["site_t"][fix["group"] == GROUP_A]), ("twin", fix["tw_t"])):
        p = pos[t]
        out[name] = {"last_round": int((p // 256 == last_round).sum()), "lane0": int((p % 64 == 0).sum()), "lane63": int((p % 64 == 63).sum()),
                     "last": int((p == fix["nd"] - 1).sum())}
    return g, out


# ---- the epilogue's solve, restated in f64 (epilogue.hip solve_body, solve.hpp rigid_gn_update / kabsch_from_sums / compose_update) --------

METRIC_WEIGHTS = {PLANE: (0.0, 1.0), POINT: (1.0, 0.0), BOTH: (0.5, 0.25)}      # (w_p2p, w_p2pl) of the GPU test's PARAMS


def _polar(L):
    U, _s, Vt = np.linalg.svd(L)
    R = U @ Vt
    assert np.linalg.det(R) > 0.0
    return R


def solve_step(metric, sums, T_cur, smt, dst_mean):
    """one outer iteration's update from the 48 sums -> (T_new as the f32 4x4 the state would hold, the step's rotation and translation in
    f64): the Gauss-Newton metrics through gn_normal_equations and a dense solve, Kabsch through an SVD, composed as compose_update does"""
    s = np.asarray(sums, np.float64)
    if metric == KABSCH:
        n = s[0]
        mud, mus = s[1:4] / n, s[4:7] / n
        sig = s[7:16].reshape(3, 3) / n - np.outer(mud, mus)
        U, _s, Vt = np.linalg.svd(sig)
        L = U @ Vt
        assert np.linalg.det(L) > 0.0
        t = mud - L @ mus
    else:
        AtA, Atb = gn_normal_equations(s, *METRIC_WEIGHTS[metric])
        dth = np.linalg.solve(AtA, Atb)
        a = dth[:3]
        na = np.sqrt(a @ a)
        u = a / na if na > 0.0 else np.zeros(3)
        c = 1.0 / np.sqrt(1.0 + na * na)
        sn = na * c
        K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
        Ra = c * np.eye(3) + sn * K + (1.0 - c) * np.outer(u, u)
        L = Ra @ Ra
        dtd = Ra @ (c * dth[3:])
        t = dtd - L @ np.asarray(smt, np.float64) + np.asarray(dst_mean, np.float64)
    R = _polar(L)
    Tc = np.asarray(T_cur, np.float32).astype(np.float64)
    Tn = np.eye(4, dtype=np.float32)
    Tn[:3, :3] = (R @ Tc[:3, :3]).astype(np.float32)
    Tn[:3, 3] = (R @ Tc[:3, 3] + t).astype(np.float32)
    return Tn, R, R @ Tc[:3, 3] + t


def assert_exact_pairs(fix, metric, T, q, smt, pairs):
    """assert_exact_fixture's conditions (1) to (3) over a pair list under T: q = T S and smt = T src_mean in f32 as in f64, the terms of
    every pair in f32 as in f64, every numerator below 2^53, the used slots non-zero and apart -> (numerators, sums)"""
    S, T = fix["S"], np.asarray(T, np.float32)
    q32 = transform_points(T, S, np.float32); q64 = transform_points(T, S, np.float64)
    assert q32.dtype == np.float32 and np.array_equal(q32, q) and np.array_equal(q32.astype(np.float64), q64), fix["name"]
    m32 = transform_points(T, fix["src_mean"].reshape(1, 3), np.float32)[0]
    assert np.array_equal(m32, smt) and np.array_equal(m32.astype(np.float64), transform_points(T, fix["src_mean"].reshape(1, 3), np.float64)[0])
    ti, si = pairs
    p, nv = fix["D"][ti], fix["N"][ti]
    z32 = pair_terms(metric, p, nv, q32[si], fix["dst_mean"], m32, np.float32)
    z64 = pair_terms(metric, p, nv, q64[si], fix["dst_mean"], m32, np.float64)
    assert z32.dtype == np.float32 and np.array_equal(z32.astype(np.float64), z64), (fix["name"], metric)
    _int_rows(z64, ZSCALE)
    df = q32[si] - p
    d2 = df[:, 0] * df[:, 0] + (df[:, 1] * df[:, 1] + df[:, 2] * df[:, 2])
    assert np.array_equal(d2.astype(np.float64), ((q64[si] - p.astype(np.float64)) ** 2).sum(1)) and np.all(d2 < fix["r2"])
    num, f64 = expected_sums_pairs(fix, metric, T, pairs)
    assert all(abs(v) < (1 << 53) for v in num) and [int(v * (1 << DEN_LOG2)) for v in f64] == num
    assert all(num[s] == 0 for s in range(NSLOTS) if s not in used_slots(metric))
    return num, f64
