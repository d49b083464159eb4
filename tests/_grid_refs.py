"""numpy restatement of the reference's voxel-grid downsamplers (helper, no tests): the yardstick of the grid-downsample
tests.  Written from the reference's own lines and from nothing in cilantro_amd/:

    core/grid_accumulator.hpp:79, :114-123     cell = floor(p * inv), inv = 1.0f / bin_size, all in f32
    core/grid_accumulator.hpp:10-39, :180-197  bins in lexicographic cell order (parallel) or in order of first appearance
    core/common_accumulators.hpp:45-46, :68-72 a sum starts AS the first member; the others are added in index order
    core/common_accumulators.hpp:122-131       if (dot(sum, n) < 0) sum -= n; else sum += n;
    core/grid_downsampler.hpp:118-126          scale = 1.0f / count; scale * sum; normals normalized()

f32 throughout.  The dot product and the squared norm are formed as x x' + (y y' + z z'), every product and sum rounded to
f32 (numpy never contracts a multiply and an add into an FMA).  Every row of `points` must be finite: a caller with
non-finite points filters them out first (the contract gives them no bin).
"""
import numpy as np

_BIAS = 1 << 20
_LOOP_MAX = 4096      # bins longer than this leave the "k-th member of every bin" loop and are folded one by one


def _dot3(a, b):
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def grid_downsample_ref(points, normals, colors, bin_size, min_points_in_bin=1, lexicographic=True, stats=None):
    """-> (points, normals or None, colors or None, counts uint32).  stats (a dict, optional) receives what the tests assert
    about the INPUT: "cells" (int64 [bins, 3], output order, before min_points_in_bin), "first" (lowest member index per bin, same
    order), "decisions" / "subtractions" of the normal rule and "min_abs_dot", the smallest |dot| any decision was taken on."""
    points = np.ascontiguousarray(points, np.float32)
    n = points.shape[0]
    assert np.isfinite(points).all()
    inv = np.float32(1.0) / np.float32(bin_size)
    cells = np.floor(points * inv).astype(np.int64)
    assert (cells >= -_BIAS).all() and (cells < _BIAS).all()
    key = ((cells[:, 0] + _BIAS) << 42) | ((cells[:, 1] + _BIAS) << 21) | (cells[:, 2] + _BIAS)
    uniq, first, inverse = np.unique(key, return_index=True, return_inverse=True)      # sorted keys = lexicographic cells
    inverse = inverse.reshape(-1)
    nb = uniq.shape[0]
    counts = np.bincount(inverse, minlength=nb).astype(np.int64)
    rest = np.ones(n, bool)
    rest[first] = False
    rest = np.nonzero(rest)[0]      # every member but the first of its bin, ascending index

    def plain_sum(a):
        s = a[first].copy()      # starts AS the first member (0.0f + -0.0f would be +0.0f)
        np.add.at(s, inverse[rest], a[rest])      # unbuffered: one f32 add at a time, in index order
        return s

    psum = plain_sum(points)
    csum = None if colors is None else plain_sum(np.ascontiguousarray(colors, np.float32))
    nsum = None
    if normals is not None:
        normals = np.ascontiguousarray(normals, np.float32)
        nsum = normals[first].copy()
        order = np.argsort(inverse, kind="stable")      # by bin, ascending index inside a bin
        start = np.concatenate(([0], np.cumsum(counts)[:-1]))
        decisions = subtractions = 0
        min_abs = np.inf
        with np.errstate(invalid="ignore", over="ignore"):
            for k in range(1, int(min(counts.max(), _LOOP_MAX))):
                b = np.nonzero(counts > k)[0]
                v = normals[order[start[b] + k]]
                d = _dot3(nsum[b], v)
                neg = d < 0
                nsum[b] = np.where(neg[:, None], nsum[b] - v, nsum[b] + v)
                decisions += b.size
                subtractions += int(neg.sum())
                if np.isfinite(d).any():
                    min_abs = min(min_abs, float(np.abs(d[np.isfinite(d)]).min()))
            for b in np.nonzero(counts > _LOOP_MAX)[0]:
                s = nsum[b].copy()
                for j in order[start[b] + _LOOP_MAX: start[b] + counts[b]]:
                    v = normals[j]
                    d = _dot3(s, v)
                    s = s - v if d < 0 else s + v
                    decisions += 1
                    subtractions += int(d < 0)
                    if np.isfinite(d):
                        min_abs = min(min_abs, abs(float(d)))
                nsum[b] = s
        if stats is not None:
            stats.update(decisions=decisions, subtractions=subtractions, min_abs_dot=min_abs)
    perm = np.arange(nb) if lexicographic else np.argsort(first, kind="stable")
    if stats is not None:
        stats.update(cells=np.stack([(uniq >> 42) - _BIAS, ((uniq >> 21) & (2 * _BIAS - 1)) - _BIAS, (uniq & (2 * _BIAS - 1)) - _BIAS], axis=1)[perm],
                     first=first[perm])
    perm = perm[counts[perm] >= min_points_in_bin]
    cnt = counts[perm]
    scale = (np.float32(1.0) / cnt.astype(np.float32))[:, None]
    out_p = scale * psum[perm]
    out_c = None if csum is None else scale * csum[perm]
    out_n = None
    if nsum is not None:
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            v = scale * nsum[perm]
            z = _dot3(v, v)
            out_n = np.where((z > 0)[:, None], v / np.sqrt(z)[:, None], v)
        assert out_n.dtype == np.float32
    assert out_p.dtype == np.float32
    return out_p, out_n, out_c, cnt.astype(np.uint32)


def explicit_loop_ref(points, normals, colors, bin_size):
    """the same contract as one member-by-member loop over the points (first-appearance order, min_points_in_bin = 1): slow, and as
    close to the reference's sequential build (grid_accumulator.hpp:186-197) as a restatement gets -- what grid_downsample_ref is
    checked against on a small cloud"""
    points = np.ascontiguousarray(points, np.float32)
    inv = np.float32(1.0) / np.float32(bin_size)
    bins, order = {}, []
    for i in range(points.shape[0]):
        c = tuple(int(np.floor(points[i, a] * inv)) for a in range(3))
        if c not in bins:
            bins[c] = [points[i].copy(), None if normals is None else normals[i].copy(), None if colors is None else colors[i].copy(), 1]
            order.append(c)
            continue
        acc = bins[c]
        acc[0] += points[i]
        if normals is not None:
            s, v = acc[1], normals[i]
            d = s[0] * v[0] + (s[1] * v[1] + s[2] * v[2])
            if d < 0:
                acc[1] = s - v
            else:
                acc[1] = s + v
        if colors is not None:
            acc[2] += colors[i]
        acc[3] += 1
    P, N, Cc, K = [], [], [], []
    for c in order:
        p, nn, cc, k = bins[c]
        scale = np.float32(1.0) / np.float32(k)
        P.append(scale * p)
        if nn is not None:
            v = scale * nn
            z = v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])
            N.append(v / np.sqrt(z) if z > 0 else v)
        if cc is not None:
            Cc.append(scale * cc)
        K.append(k)
    f = lambda rows: np.array(rows, np.float32).reshape(-1, 3)      # noqa: E731
    return f(P), (f(N) if normals is not None else None), (f(Cc) if colors is not None else None), np.array(K, np.uint32)
