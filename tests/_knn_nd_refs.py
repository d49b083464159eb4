"""The yardstick of DESIGN.md section 21: rules N1 to N5 in numpy float32, one rounding per operation, and a lexsort on (d2, index).
Nothing here runs on a device or calls the library."""
import numpy as np

NONE = 0xFFFFFFFF
TILE = 4      # KNN_ND_TILE of csrc/knn_nd.hip (tests/test_knn_nd_refs_cpu.py checks that the source still says so)


def d2_matrix(ref, qry):
    """N1 -> [nq, nr] float32: r = 0; r = r + (((s0 + s1) + s2) + s3) per full group of four; r = r + s for each coordinate left over"""
    ref = np.ascontiguousarray(ref, np.float32)
    qry = np.ascontiguousarray(qry, np.float32)
    dim = ref.shape[1]
    assert qry.shape[1] == dim
    with np.errstate(over="ignore", invalid="ignore"):
        def s(d):
            t = qry[:, None, d] - ref[None, :, d]      # float32 - float32: one rounding
            return t * t

        r = np.zeros((len(qry), len(ref)), np.float32)
        d = 0
        while d + 4 <= dim:
            r = r + (((s(d) + s(d + 1)) + s(d + 2)) + s(d + 3))
            d += 4
        while d < dim:
            r = r + s(d)
            d += 1
    assert r.dtype == np.float32
    return r


def _sorted_rows(d2, bound):
    """per query: the accepted candidates (N2) ascending by (d2, index) (N3) -> list of (idx int64, d2 f32)"""
    out = []
    for row in d2:
        ok = np.isfinite(row) & (row < np.float32(bound))
        cand = np.nonzero(ok)[0]
        order = np.lexsort((cand, row[cand]))
        out.append((cand[order].astype(np.int64), row[cand][order]))
    return out


def knn(ref, qry, k, max_sq_dist=np.inf):
    """-> (idx int64 [nq, k] padded with -1, d2 f32 [nq, k] padded with +inf, counts int64 [nq]); qry None: self search"""
    ref = np.ascontiguousarray(ref, np.float32)
    qry = ref if qry is None else np.ascontiguousarray(qry, np.float32)
    idx = np.full((len(qry), k), -1, np.int64)
    dd = np.full((len(qry), k), np.inf, np.float32)
    cnt = np.zeros(len(qry), np.int64)
    if len(ref) and len(qry):
        for i, (ci, cd) in enumerate(_sorted_rows(d2_matrix(ref, qry), max_sq_dist)):
            m = min(k, len(ci))
            idx[i, :m], dd[i, :m], cnt[i] = ci[:m], cd[:m], m
    return idx, dd, cnt


def radius(ref, qry, radius_sq):
    """N5 -> (offsets int64 [nq + 1], idx int64 [total], d2 f32 [total])"""
    ref = np.ascontiguousarray(ref, np.float32)
    qry = ref if qry is None else np.ascontiguousarray(qry, np.float32)
    off = np.zeros(len(qry) + 1, np.int64)
    ii, dd = [np.zeros(0, np.int64)], [np.zeros(0, np.float32)]
    if len(ref) and len(qry) and radius_sq > 0:
        for i, (ci, cd) in enumerate(_sorted_rows(d2_matrix(ref, qry), radius_sq)):
            off[i + 1] = len(ci)
            ii.append(ci); dd.append(cd)
    return np.cumsum(off), np.concatenate(ii), np.concatenate(dd)


def cloud(n, dim, seed, centre=5.0):
    """the fixtures' clouds: standard normal around (centre, ..., centre)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, dim)) + centre).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
