"""What the searches must return on clouds that hold NaN / +-inf points (c_api.h, "Non-finite points"): a point with a non-finite
coordinate keeps its index, is never a neighbour and finds nothing as a query; everybody else gets what the same call returns on
the clouds with those rows removed, indices mapped back.

    spoil()        writes non-finite values into chosen rows
    expected_*()   the existing oracle calls on the FILTERED clouds, indices mapped back to the unfiltered ones
    brute_*()      a few lines of numpy in f32 on the UNFILTERED arrays (IEEE comparisons: a NaN or infinite squared distance is
                   never < the radius): what tests/test_nonfinite_refs_cpu.py holds the expected_*() helpers against
"""
import numpy as np

KINDS = ("nan_one", "nan_all", "pos_inf", "neg_inf", "pos_inf_x_neg_inf_y")


def spoil(cloud, rows, kinds):
    """copy of `cloud` with row rows[i] spoiled the kinds[i % len(kinds)] way; kinds: names from KINDS (or one name)"""
    out = np.array(cloud, dtype=np.float32, copy=True)
    if isinstance(kinds, str):
        kinds = (kinds,)
    for i, r in enumerate(np.asarray(rows, dtype=np.int64)):
        kind = kinds[i % len(kinds)]
        if kind == "nan_one":
            out[r, (i // len(kinds)) % 3] = np.nan
        elif kind == "nan_all":
            out[r, :] = np.nan
        elif kind == "pos_inf":
            out[r, (i // len(kinds)) % 3] = np.inf
        elif kind == "neg_inf":
            out[r, (i // len(kinds)) % 3] = -np.inf
        elif kind == "pos_inf_x_neg_inf_y":
            out[r, 0] = np.inf
            out[r, 1] = -np.inf
        else:
            raise ValueError(kind)
    return out


def spoiled_rows(n, which, seed=5):
    """the row sets of the tests: 'first', 'last', 'run' (70 consecutive rows: longer than a wave), 'random' (5 %), 'mixed' (all of them)"""
    rng = np.random.default_rng(seed)
    first, last = np.array([0]), np.array([n - 1])
    run = np.arange(n // 3, min(n // 3 + 70, n))
    rnd = np.sort(rng.choice(n, max(1, n // 20), replace=False))
    return {"first": first, "last": last, "run": run, "random": rnd, "mixed": np.unique(np.concatenate([first, last, run, rnd]))}[which]


def finite_mask(cloud):
    return np.all(np.isfinite(np.asarray(cloud, np.float32).reshape(-1, 3)), axis=1)


def _kept(cloud):
    m = finite_mask(cloud)
    return m, np.nonzero(m)[0].astype(np.int64)


# ---- expectations: the oracle on the filtered clouds ---------------------------------------------------------------------------
def expected_nn(orc, dst, q, max_sq):
    """SECOND_TO_FIRST -> (dst_idx, src_idx, d2) in ascending src order, and per query (nn_idx, -1 = none; nn_d2, valid where found)"""
    md, kd = _kept(dst)
    mq, kq = _kept(q)
    nn = np.full(len(q), -1, np.int64)
    nd2 = np.zeros(len(q), np.float32)
    if len(kd) == 0 or len(kq) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), nn, nd2
    di, si, dv = orc.KDTree(dst[md]).find_correspondences(q[mq], float(max_sq))
    di, si = kd[di], kq[si]
    nn[si] = di
    nd2[si] = dv
    return di, si, dv, nn, nd2


def expected_dir(orc, dst, q, max_sq, direction, reciprocal=False):
    """search directions 1 / 2 -> (dst_idx, src_idx, d2); both index maps are monotone, so the lexicographic (first, second) order survives"""
    md, kd = _kept(dst)
    mq, kq = _kept(q)
    if len(kd) == 0 or len(kq) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32)
    di, si, dv = orc.find_correspondences_dir(dst[md], q[mq], float(max_sq), direction, reciprocal)
    return kd[di], kq[si], dv


def expected_knn(orc, ref, q, k, radius_sq=np.inf):
    """-> (idx int64 [nq, k] -1 padded, d2 [nq, k] +inf padded, counts); q None: the reference cloud's own points"""
    q = ref if q is None else q
    mr, kr = _kept(ref)
    mq, kq = _kept(q)
    idx = np.full((len(q), k), -1, np.int64)
    d2 = np.full((len(q), k), np.inf, np.float32)
    cnt = np.zeros(len(q), np.int64)
    if len(kr) and len(kq):
        oi, od, oc = orc.knn_batch(orc.KDTree(ref[mr]), q[mq], k, radius_sq)
        idx[kq] = np.where(oi >= 0, kr[np.maximum(oi, 0)], -1)
        d2[kq] = od
        cnt[kq] = oc
    return idx, d2, cnt


def expected_radius(orc, ref, q, radius_sq):
    """-> (offsets int64 [nq + 1], idx, d2): lists in (d2, index) order; the map is monotone, so the order among equal distances survives"""
    q = ref if q is None else q
    mr, kr = _kept(ref)
    mq, kq = _kept(q)
    cnt = np.zeros(len(q), np.int64)
    if len(kr) and len(kq):
        ooff, oidx, od2 = orc.radius_search(ref[mr], q[mq], radius_sq)
        cnt[kq] = np.diff(ooff)
        idx, d2 = kr[oidx], od2
    else:
        idx, d2 = np.zeros(0, np.int64), np.zeros(0, np.float32)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)      # (spoiled queries own empty lists: the concatenation is unchanged)
    return off, idx, d2


# ---- brute force on the unfiltered arrays: proves the helpers above, not the kernels ---------------------------------------------
def brute_d2(ref, q):
    """[nq, nref] f32, the pinned ((dx*dx)+(dy*dy))+(dz*dz); NaN / inf where either point is not finite"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = q[:, None, :].astype(np.float32) - ref[None, :, :].astype(np.float32)
        return ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])


def brute_lists(ref, q, radius_sq, k=None):
    """per query: indices of the points with d2 < radius_sq (false on NaN, and on inf whatever the radius), by (d2, index), the first k"""
    D = brute_d2(ref, q)
    out = []
    for row in D:
        with np.errstate(invalid="ignore"):
            ok = np.nonzero(row < np.float32(radius_sq))[0]      # (IEEE: NaN < r and inf < inf are false)
        ok = ok[np.lexsort((ok, row[ok]))]
        out.append((ok[:k] if k is not None else ok, row[ok][:k] if k is not None else row[ok]))
    return out


def tie_free(ref, q, radius_sq, k):
    """brute force: no two of a query's k + 1 nearest in-range distances are equal (its nearest and its k-th are unique)"""
    return all(len(np.unique(d2)) == len(d2) for _, d2 in brute_lists(ref, q, radius_sq, k + 1))


def tie_free_oracle(orc, ref, q, radius_sq, k):
    """the same for the full-size inputs, from the oracle's lists over the finite rows (k + 1 <= 64)"""
    _, d2, cnt = expected_knn(orc, ref, q, k + 1, radius_sq)
    live = np.arange(1, k + 1)[None, :] < cnt[:, None]
    return not ((d2[:, 1:] == d2[:, :-1]) & live).any()


# ---- the inputs of tests/test_gpu_nonfinite.py (tests/test_nonfinite_refs_cpu.py shows that they are tie-free) ---------------------
PAIR_SIZES = (20000, 2049, 257)
ROW_SETS = ("first", "last", "run", "random", "mixed")


def pair_case(orc, n, dst_rows=None, src_rows=None):
    """the synthetic pair under its true transform; dst_rows / src_rows: a name from ROW_SETS (all five kinds mixed over the rows) or None
    -> dict(dst, src, T (4x4 f32), q = fl(T src), max_sq, h)"""
    from cilantro_amd import synthetic as syn

    d = syn.make_pair(n, perturb=0.5)
    dst, src = d["dst"], d["src"]
    if dst_rows is not None:
        dst = spoil(dst, spoiled_rows(n, dst_rows, seed=5), KINDS)
    if src_rows is not None:
        src = spoil(src, spoiled_rows(n, src_rows, seed=6), KINDS)
    T = d["T_true"].astype(np.float32)
    return {"dst": np.ascontiguousarray(dst), "src": np.ascontiguousarray(src), "T": T, "q": orc.transform_points(T, src), "max_sq": np.float32(d["max_sq_dist"]),
            "h": d["h"]}


def hostile_case(orc, n=20000):
    """finite but hostile: two far outliers in the target, the same two in the source moved by half the search radius along x (both have
    in-range matches): the grid collapses to a few huge cells"""
    c = pair_case(orc, n)
    far = np.float32([[1e6, 0, 0], [-3e5, 2e5, 7e5]])
    c["dst"] = np.ascontiguousarray(np.concatenate([c["dst"], far]))
    shift = np.float32([0.5 * np.sqrt(np.float64(c["max_sq"])), 0, 0])
    Ti = np.linalg.inv(c["T"].astype(np.float64))
    want = far.astype(np.float64) + shift
    far_src = ((want @ Ti[:3, :3].T) + Ti[:3, 3]).astype(np.float32)
    # (at 1e6 one f32 ulp is a tenth of the search radius: of the f32 points around the exact pre-image take the one whose image under the
    #  pinned f32 transform lands nearest to the intended place)
    steps = np.stack(np.meshgrid(*([np.arange(-2, 3)] * 3), indexing="ij"), -1).reshape(-1, 3)
    for i in range(len(far_src)):
        cand = (far_src[i][None, :] + steps * np.spacing(np.abs(far_src[i]))[None, :]).astype(np.float32)
        err = ((orc.transform_points(c["T"], cand).astype(np.float64) - want[i]) ** 2).sum(axis=1)
        far_src[i] = cand[int(err.argmin())]
    c["src"] = np.ascontiguousarray(np.concatenate([c["src"], far_src]))
    c["q"] = orc.transform_points(c["T"], c["src"])
    return c
