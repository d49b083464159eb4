"""Fixtures and a plain numpy restatement for the engine's post-filters and pair lists (filters.hip, bidir.hip, the getter of
c_api.hip): inlier_fraction, one_to_one, the search directions FIRST_TO_SECOND / BOTH and require_reciprocality.

Fixtures.  Every coordinate is a multiple of 2^-10 with magnitude below 2^6, so every subtraction, square and sum of the pinned
d2 of a MATCH is exact in f32 (a match is `a` units of 2^-10 off a lattice point along one axis: d2 = a^2 * 2^-20), and the
transforms of TRANSFORMS keep it exact: the source handed to the library is T^-1 of the fixture's `q`, and T * that is `q` again, bit
for bit.  The generators are seeded and vectorised; original indices are shuffled, so index order is not grid order.  Each
generator also returns the two directed correspondence sets BY CONSTRUCTION (`fwd`: source -> nearest target, ascending source
index; `rev`: target -> nearest source, ascending target index; None where that search would meet a nearest-neighbour tie), so that
a large case needs no CPU search; tests/test_filter_refs_cpu.py holds them against brute force at the small sizes.

Restatement.  Over (first, second, d2) triples: the fraction filter (llround as the C expression on doubles), one-to-one in both
branches of core/correspondence.hpp:68-100, union / intersection of the two directed sets, and the order the reference leaves
(oracle/icp_oracle.h:62-66).  tests/test_filter_refs_cpu.py pins every function to the oracle's."""
import math

import numpy as np

UNIT = 2.0 ** -10
STEP = 128                                            # lattice spacing 2^-3, in units
MAX_SQ_ATTACHED = np.float32(24 * 24 * 2.0 ** -20)    # a = 24 sits exactly ON the radius: the comparison is strict
MAX_SQ_SHARED = np.float32(72 * 72 * 2.0 ** -20)
COUNT_PROBS = (0.07, 0.12, 0.15, 0.25, 0.41)          # a target gets 0, 1, 2, 3 or 5 sources: 3.22 on average
S2F, F2S, BOTH = 0, 1, 2                              # search_direction option codes (SECOND_TO_FIRST is the default)

COUNTS = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257)      # forward matches the attached fixture is cut to
FRACTIONS = (1e-9, 0.999999, 0.5, 1.0, 0.0)           # + half_fractions(n) of the list at hand


def bits(d2):
    return np.ascontiguousarray(d2, np.float32).view(np.uint32)


def _d2_of(a):
    """a^2 * 2^-20 (exact: a < 2^12)"""
    return (np.asarray(a, np.int64) ** 2 * 2.0 ** -20).astype(np.float32)


def _triple(first, second, a, by):
    first = np.asarray(first, np.int64); second = np.asarray(second, np.int64)
    o = np.argsort(second if by == "second" else first, kind="stable")
    return first[o], second[o], _d2_of(a)[o]


def _lattice(nx, ny, nz, origin):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)
    return g * STEP + np.asarray(origin, np.int64)


def _cloud(units, perm=None):
    x = (units * UNIT).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) / UNIT, units) and np.abs(units).max(initial=0) < 2 ** 16
    if perm is None:
        return x
    out = np.empty_like(x)
    out[perm] = x
    return out


# ---- fixtures --------------------------------------------------------------------------------------------------------

def attached(side, seed, planar=False, tied=False):
    """Targets on a cubic lattice of spacing 2^-3 (planar: one layer at z = 0); each source is its target +- a * 2^-10 along one axis,
    0 <= a < 32.  A target gets 0, 1, 2, 3 or 5 sources: one with the strictly smallest a (the reverse nearest neighbour is unique), the
    others in pairs of equal a on different axes (value ties that are not the minimum; with 2 sources, one single other).  a < 24
    matches, a = 24 lies exactly on the radius, a > 24 is out of reach.
    tied (`tied_minima`, SECOND_TO_FIRST only): half the targets with 2+ sources have 2 to 4 sources at the SAME smallest a (a >= 1,
    distinct places): the one-to-one tie-break "lowest source index" decides; rev is None."""
    rng = np.random.default_rng(seed)
    nax = 2 if planar else 3
    tgt = _lattice(side, side, 1 if planar else side, (-3 * STEP + 17, 5 * STEP - 40, 0 if planar else -2 * STEP + 5))
    nd = len(tgt)
    cnt = rng.choice(np.array([0, 1, 2, 3, 5]), size=nd, p=COUNT_PROBS)
    a = np.empty((nd, 5), np.int64)
    # (small a more often than large: about 87 % of the sources match, 2 % lie on the radius, 11 % beyond it)
    a[:, 0] = np.maximum(rng.integers(0, 30, nd) * rng.integers(0, 30, nd) // 29, 1 if tied else 0)
    a[:, 1] = a[:, 2] = a[:, 0] + 1 + rng.integers(0, 31 - a[:, 0]) // 2
    a[:, 3] = a[:, 4] = rng.integers(a[:, 0] + 1, 32)
    axis = np.empty((nd, 5), np.int64)
    sign = rng.choice(np.array([-1, 1]), size=(nd, 5))
    axis[:, 0] = rng.integers(0, nax, nd)
    for p in (1, 3):
        axis[:, p] = rng.integers(0, nax, nd)
        axis[:, p + 1] = (axis[:, p] + 1 + rng.integers(0, nax - 1, nd)) % nax
    if tied:
        assert not planar
        pick = (cnt >= 2) & (rng.random(nd) < 0.5)
        n_same = np.where(pick, np.minimum(cnt, rng.integers(2, 5, nd)), 1)
        c0 = rng.integers(0, 6, nd)
        for j in range(4):
            sel = pick & (j < n_same)
            combo = (c0 + j) % 6                      # six places at distance a: distinct for j = 0..3
            a[sel, j] = a[sel, 0]; axis[sel, j] = combo[sel] // 2; sign[sel, j] = 2 * (combo[sel] % 2) - 1
    rows, slots = np.nonzero(np.arange(5)[None, :] < cnt[:, None])
    av = a[rows, slots]
    pos = tgt[rows].copy()
    pos[np.arange(len(rows)), axis[rows, slots]] += sign[rows, slots] * av
    ns = len(rows)
    perm_t = rng.permutation(nd); perm_s = rng.permutation(ns)
    owner = np.empty(ns, np.int64)
    owner[perm_s] = perm_t[rows]
    hit = av < 24
    first_slot = (slots == 0) & hit
    return {"name": ("tied_minima" if tied else "attached_planar" if planar else "attached") + f"_{side}",
            "dst": _cloud(tgt, perm_t), "q": _cloud(pos, perm_s), "max_sq": MAX_SQ_ATTACHED, "owner": owner,
            "fwd": _triple(perm_t[rows[hit]], perm_s[hit], av[hit], "second"),
            "rev": None if tied else _triple(perm_t[rows[first_slot]], perm_s[first_slot], av[first_slot], "first"),
            "on_radius": int((av == 24).sum())}


def shared(side, seed, midpoint=False):
    """Targets in pairs (A, B = A + one lattice step along x).  45 % of the pairs share ONE source, 60 * 2^-10 from A towards B: B has
    no source of its own and names the same one at 68 * 2^-10 (max_sq = 72^2 * 2^-20).  35 % hold up to one source of their own each,
    +- a * 2^-10 along y or z (0 <= a < 32), the rest none.  midpoint (FIRST_TO_SECOND only): the shared source sits at 64 * 2^-10, the
    exact midpoint -- equal values, the lowest target index must win one-to-one; fwd is None (the forward search would tie)."""
    assert side % 2 == 0
    rng = np.random.default_rng(seed)
    ta = _lattice(side // 2, side, side, (5 * STEP + 9, -4 * STEP - 21, 2 * STEP + 3))
    ta[:, 0] = (ta[:, 0] - (5 * STEP + 9)) * 2 + (5 * STEP + 9)          # every other lattice point along x
    tb = ta + np.array([STEP, 0, 0])
    npair = len(ta)
    tgt = np.concatenate([ta, tb])
    kind = rng.choice(np.array([0, 1, 2]), size=npair, p=(0.2, 0.45, 0.35))
    off = 64 if midpoint else 60
    sh = np.nonzero(kind == 1)[0]
    f1, s1, a1, pos = [], [], [], []                   # reverse matches (target grid index, source build index, a)
    pos.append(ta[sh] + np.array([off, 0, 0]))
    k0 = np.arange(len(sh))
    f1 += [sh, sh + npair]; s1 += [k0, k0]; a1 += [np.full(len(sh), off), np.full(len(sh), STEP - off)]
    nb = len(sh)
    for half, base in ((0, ta), (1, tb)):
        own = np.nonzero((kind == 2) & (rng.random(npair) < 0.7))[0]
        ao = rng.integers(0, 32, len(own))
        p = base[own].copy()
        p[np.arange(len(own)), rng.integers(1, 3, len(own))] += rng.choice(np.array([-1, 1]), size=len(own)) * ao
        pos.append(p)
        f1.append(own + half * npair); s1.append(nb + np.arange(len(own))); a1.append(ao)
        nb += len(own)
    pos = np.concatenate(pos); f1 = np.concatenate(f1); s1 = np.concatenate(s1); a1 = np.concatenate(a1)
    perm_t = rng.permutation(len(tgt)); perm_s = rng.permutation(len(pos))
    rev = _triple(perm_t[f1], perm_s[s1], a1, "first")
    nearer = ~((f1 >= npair) & (s1 < len(sh)))         # every reverse match but B's of a shared source is the source's own nearest target
    return {"name": ("shared_midpoint" if midpoint else "shared") + f"_{side}", "dst": _cloud(tgt, perm_t), "q": _cloud(pos, perm_s),
            "max_sq": MAX_SQ_SHARED, "rev": rev, "fwd": None if midpoint else _triple(perm_t[f1[nearer]], perm_s[s1[nearer]], a1[nearer], "second"),
            "shared_sources": int(len(sh))}


def _keep_families(fix, fam_keep, tag):
    """the attached fixture without the sources of some targets (a target's sources go together: the reverse matches stay unique)"""
    keep_s = fam_keep[fix["owner"]]
    new_idx = np.cumsum(keep_s) - 1

    def remap(t):
        if t is None:
            return None
        m = keep_s[t[1]]
        return t[0][m], new_idx[t[1][m]], t[2][m]

    out = dict(fix)
    out.update(name=fix["name"] + tag, q=np.ascontiguousarray(fix["q"][keep_s]), owner=fix["owner"][keep_s], fwd=remap(fix["fwd"]), rev=remap(fix["rev"]))
    out.pop("on_radius", None)
    return out


def _greedy(weight, always, total):
    keep = always.copy()
    left = total
    for t in np.nonzero(~always)[0]:
        if left == 0:
            break
        if weight[t] <= left:
            keep[t] = True
            left -= weight[t]
    assert left == 0, (total, left)
    return keep


def cut_matches(fix, m):
    """exactly m forward matches: every family without one, and families in target-index order while they fit"""
    nd = len(fix["dst"])
    hits = np.bincount(fix["fwd"][0], minlength=nd)
    size = np.bincount(fix["owner"], minlength=nd)
    out = _keep_families(fix, _greedy(hits, (hits == 0) & (size > 0), m), f"_m{m}")
    assert len(out["fwd"][0]) == m and len(out["q"]) > 0
    return out


def cut_sources(fix, ns):
    """exactly ns sources, by whole families in target-index order"""
    size = np.bincount(fix["owner"], minlength=len(fix["dst"]))
    out = _keep_families(fix, _greedy(size, size == 0, ns), f"_s{ns}")
    assert len(out["q"]) == ns
    return out


# ---- exact transforms ------------------------------------------------------------------------------------------------

def _T(L, t=(0, 0, 0)):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = L; T[:3, 3] = t
    return T


# name -> (T, inverse of its linear part or None: singular)
TRANSFORMS = {
    "identity": (_T(np.eye(3)), np.eye(3)),
    "rz90_shift": (_T([[0, -1, 0], [1, 0, 0], [0, 0, 1]], (3, -2, 5)), np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float64)),
    "mirror_z": (_T(np.diag([1, 1, -1])), np.diag([1.0, 1.0, -1.0])),
    "scale_2": (_T(np.diag([2, 2, 2])), np.diag([0.5, 0.5, 0.5])),
    "flatten_z": (_T(np.diag([1, 1, 0])), None),       # over a planar fixture: find_pairs' transformed-copy branch
}


def stored_source(q, name, seed=0):
    """s with T s == q exactly: T^-1 q (exact: permutations, sign flips, integer shifts, halving); for the singular diag(1, 1, 0) q is
    planar (z = 0) and s gets arbitrary z, multiples of 2^-10 in (-8, 8)"""
    T, Linv = TRANSFORMS[name]
    q64 = q.astype(np.float64)
    if Linv is None:
        assert not q64[:, 2].any()
        s64 = q64.copy()
        s64[:, 2] = np.random.default_rng(seed).integers(-8191, 8192, len(q)) * UNIT
    else:
        s64 = (q64 - T[:3, 3].astype(np.float64)) @ Linv.T
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64)
    return np.ascontiguousarray(s)


# ---- the restatement -------------------------------------------------------------------------------------------------

def keep_count(fraction, n):
    """(size_t)llround(fraction * (double)n), core/correspondence.hpp:63: half away from zero -- not Python's round()"""
    x = float(fraction) * float(n)
    k = math.floor(x)
    if x - k >= 0.5:
        k += 1
    return min(int(k), int(n))


def half_fractions(n):
    """up to two fractions f in (0, 1), near 1/4 and 3/4, for which the double product f * n is EXACTLY an integer plus one half"""
    out = []
    for near in (0.25, 0.75):
        k0 = int(near * n)
        for k in sorted(range(max(0, k0 - 64), min(n, k0 + 65)), key=lambda k: abs(k - k0)):
            f = (2 * k + 1) / (2.0 * n)
            if 0.0 < f < 1.0 and f * float(n) == k + 0.5 and f not in out:
                out.append(f)
                break
    return out


def _take(t, o):
    return t[0][o], t[1][o], t[2][o]


def _filtering(fraction):
    return 0.0 < fraction < 1.0                        # correspondence.hpp:60


def fraction_s2f(t, fraction):
    """filterCorrespondencesFraction on a SECOND_TO_FIRST set: the llround(f n) smallest by (bits(d2), source index), in that order"""
    if not _filtering(fraction):
        return t
    o = np.lexsort((t[1], bits(t[2])))
    return _take(t, o[:keep_count(fraction, len(o))])


def fraction_pairs(t, fraction):
    """... on a pair list: the smallest by (bits(d2), first, second), in that order"""
    if not _filtering(fraction):
        return t
    o = np.lexsort((t[1], t[0], bits(t[2])))
    return _take(t, o[:keep_count(fraction, len(o))])


def _first_of_runs(key):
    return np.concatenate([[True], key[1:] != key[:-1]]) if len(key) else np.zeros(0, bool)


def one_to_one_s2f(t):
    """correspondence.hpp:84-95: per target the smallest value (ties: lowest source index); ordered by target index"""
    o = np.lexsort((t[1], bits(t[2]), t[0]))
    return _take(t, o[_first_of_runs(t[0][o])])


def one_to_one_f2s(t):
    """correspondence.hpp:72-82: per source the smallest value (ties: lowest target index); ordered by source index"""
    o = np.lexsort((t[0], bits(t[2]), t[1]))
    return _take(t, o[_first_of_runs(t[1][o])])


def _key(t):
    return (t[0] << 32) | t[1]


def union(a, b):
    """std::set_union of two sets sorted by (first, second): an element of `a` wins on equality"""
    c = tuple(np.concatenate([x, y]) for x, y in zip(a, b))
    _, o = np.unique(_key(c), return_index=True)       # (first occurrence: a's)
    return _take(c, o)


def intersection(a, b):
    """std::set_intersection: the elements of `a` that `b` holds too"""
    _, ia, _ = np.intersect1d(_key(a), _key(b), assume_unique=True, return_indices=True)
    return _take(a, ia)


def contended(t, col):
    """(indices of column `col` that two or more entries name, those whose SMALLEST value two or more entries hold): what one-to-one decides"""
    if len(t[0]) == 0:
        return 0, 0
    o = np.lexsort((bits(t[2]), t[col]))
    k, v = t[col][o], bits(t[2])[o]
    start = _first_of_runs(k)
    run = np.cumsum(start) - 1
    size = np.bincount(run)
    at_min = np.bincount(run, weights=(v == v[np.nonzero(start)[0]][run]))
    return int((size >= 2).sum()), int((at_min >= 2).sum())


def expected(fix, direction, reciprocal=False, fraction=1.0, one_to_one=False):
    """the list get_correspondences must return: (first, second, d2) in the order the reference leaves (oracle/icp_oracle.h:62-66)"""
    if direction == S2F:
        t = fraction_s2f(fix["fwd"], fraction)
        return one_to_one_s2f(t) if one_to_one else t
    if direction == F2S:
        t = fix["rev"]
    else:                                              # the reverse set is the first argument of set_union / set_intersection
        t = intersection(fix["rev"], fix["fwd"]) if reciprocal else union(fix["rev"], fix["fwd"])
    t = fraction_pairs(t, fraction)
    return one_to_one_f2s(t) if (one_to_one and direction == F2S) else t      # BOTH: one-to-one is a no-op (:96-98)


def same(got, exp):
    """element for element: indices and the distances' bits"""
    return (len(got[0]) == len(exp[0]) and np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
            and np.array_equal(bits(got[2]), bits(exp[2])))
