"""Plain numpy references for the model kernels' exact quantities (test infrastructure; pinned by test_model_refs_cpu.py).

KMeans: the product documents its cluster sums as exact fixed-point integers at scale 2^S (kmeans.hip), so the
reference is integer arithmetic, not a tolerance:
    f = rint(float64(x) * 2^S)      (a power-of-two scaling of an f32 value is exact in f64; rint rounds half to even like llrint)
    sums[j] = sum of int64(f) over the points labelled j, counts alongside
    centroid = float32(float64(sum) / 2^S / count)                (the product's documented formula)
A non-finite coordinate has no integer image: it is left out of the integer sum (its point still counts) and the centroid's
coordinate is what an IEEE sum of the cluster would give -- NaN if the cluster holds a NaN or both infinities, else the infinity.
"""
import numpy as np

NF_NAN, NF_PINF, NF_NINF = 1, 2, 4      # per cluster and coordinate d: flag << (3 * d)


def fixed_point(x, S):
    """int64 image of f32 coordinates at scale 2^S; non-finite coordinates -> 0"""
    v = np.asarray(x, np.float32).astype(np.float64) * float(np.ldexp(1.0, int(S)))
    v = np.where(np.isfinite(v), v, 0.0)
    return np.rint(v).astype(np.int64)


def kmeans_sums(x, labels, k, S):
    """-> int64 [k, 4]: {sum x, sum y, sum z (fixed point, 2^S), count} per label, in integer arithmetic"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64)
    out = np.zeros((k, 4), np.int64)
    if len(x) == 0:
        return out
    f = fixed_point(x, S)
    order = np.argsort(labels, kind="stable")
    cnt = np.bincount(labels, minlength=k).astype(np.int64)      # (unweighted: integer counts)
    ends = np.cumsum(cnt)
    cs = np.concatenate([np.zeros((1, 3), np.int64), np.cumsum(f[order], axis=0, dtype=np.int64)])
    out[:, :3] = cs[ends] - cs[ends - cnt]
    out[:, 3] = cnt
    return out


def kmeans_nonfinite_flags(x, labels, k):
    """-> uint32 [k]: bits NF_* << (3 * d) for every cluster that holds a NaN / +inf / -inf in coordinate d"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64)
    fl = np.zeros(k, np.uint32)
    rows = np.nonzero(~np.isfinite(x).all(axis=1))[0]
    for i in rows:
        for d in range(3):
            v = x[i, d]
            b = NF_NAN if np.isnan(v) else (NF_PINF if v == np.inf else (NF_NINF if v == -np.inf else 0))
            fl[labels[i]] |= np.uint32(b << (3 * d))
    return fl


def centroids_from_sums(sums, S, flags=None):
    """float32(float64(sum) / 2^S / count) per coordinate; count 0 -> NaN (0 / 0), like the product's host step"""
    sums = np.asarray(sums, np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (sums[:, :3].astype(np.float64) / float(np.ldexp(1.0, int(S))) / sums[:, 3:4].astype(np.float64)).astype(np.float32)
    if flags is not None:
        for j in np.nonzero(np.asarray(flags))[0]:
            for d in range(3):
                b = (int(flags[j]) >> (3 * d)) & 7
                if b & NF_NAN or (b & NF_PINF and b & NF_NINF):
                    c[j, d] = np.nan
                elif b & NF_PINF:
                    c[j, d] = np.inf
                elif b & NF_NINF:
                    c[j, d] = -np.inf
    return c


def scale_for(x):
    """the product's scale exponent for a whole cloud: from the largest FINITE |coordinate| and the point count"""
    from cilantro_amd.distributed_models import scale_exponent

    x = np.asarray(x, np.float32)
    a = np.abs(x[np.isfinite(x)])
    return scale_exponent(float(a.max()) if a.size else 0.0, x.reshape(-1, 3).shape[0])


def farthest_key(x, labels, cluster, centre, index_offset=0):
    """HipKMeansShard.farthest: max over the cluster's points of bits(d) << 32 | (0xFFFFFFFF - global index), d the pinned f32
    d0*d0 + (d1*d1 + d2*d2) with d = centre - x; 0 for an empty cluster.  The maximum prefers the lowest index among equal d."""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    m = np.nonzero(np.asarray(labels) == cluster)[0]
    if len(m) == 0:
        return 0
    c = np.asarray(centre, np.float32).reshape(3)
    d = c[None, :] - x[m]
    sq = d * d
    dist = (sq[:, 0] + (sq[:, 1] + sq[:, 2])).astype(np.float32)
    key = (dist.view(np.uint32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - (m.astype(np.uint64) + np.uint64(index_offset)))
    return int(key.max())


def lloyd_step(x, labels, centroids, S, with_flags=True):
    """One host step of ShardedKMeans3f.cluster on the integers, given the labels of the assignment under `centroids`: the empty-
    cluster repair (kmeans.hpp:134-176: the farthest member of the largest cluster moves, its coordinates leave that cluster's sum
    and are NOT added to the empty one's), then the new centroids.  -> (centroids f32 [k,3], labels after the repair, sums)"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    labels = np.asarray(labels, np.int64).copy()
    k = len(centroids)
    hs = kmeans_sums(x, labels, k, S)
    scale = float(np.ldexp(1.0, int(S)))
    flags = kmeans_nonfinite_flags(x, labels, k) if with_flags else None      # (of the assignment pass, as the product records them)
    for i in range(k):
        if hs[i, 3] != 0:
            continue
        mx = int(np.argmax(hs[:, 3]))
        oc = (hs[mx, :3].astype(np.float64) / scale / np.float64(hs[mx, 3])).astype(np.float32)
        key = farthest_key(x, labels, mx, oc)
        gi = 0xFFFFFFFF - (key & 0xFFFFFFFF)
        labels[gi] = i
        hs[mx, :3] -= fixed_point(x[gi], S)
        hs[mx, 3] -= 1
        hs[i, 3] += 1
    return centroids_from_sums(hs, S, flags), labels, hs
