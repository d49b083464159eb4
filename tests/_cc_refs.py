"""numpy restatements of connected-component segmentation, the yardstick of tests/test_gpu_components.py:

  serial_reference()   a literal serial transcription of clustering/connected_component_extraction.hpp:162-265 of the reference -- the
                       skip of list entry 0, the merge sets, the max_segment_size fill rule, the size sort (made stable) -- over brute-force
                       f32 neighbour lists; a few thousand points at the most
  fast_components()    rules 1-4 of the contract restated as a union-find over a grid-hashed pair list, for larger clouds

Both evaluate the clauses with the pinned f32 arithmetic of rule 3 (numpy rounds every f32 operation and fuses nothing).
tests/test_components_refs_cpu.py pins the two against each other (and the second against scipy where it is installed)."""
import numpy as np

F32 = np.float32


class Clauses:
    """the three clauses of rule 3, selected independently (None: not selected)"""

    def __init__(self, max_distance=None, normals=None, max_angle=None, angle_inclusive=False, colors=None, color_thresh=None):
        self.max_distance = None if max_distance is None else F32(max_distance)
        self.normals = None if normals is None else np.ascontiguousarray(normals, F32)
        self.max_angle = None if max_angle is None else F32(max_angle)
        self.angle_inclusive = bool(angle_inclusive)
        self.colors = None if colors is None else np.ascontiguousarray(colors, F32)
        self.color_thresh = None if color_thresh is None else F32(color_thresh)


def d2_pinned(p, i, j):
    """((dx*dx)+(dy*dy))+(dz*dz), every operation rounded to f32"""
    d = p[i] - p[j]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def dot_pinned(a, b):
    """x*x' + (y*y' + z*z')"""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def pair_angle(nrm, i, j):
    with np.errstate(invalid="ignore"):
        return np.arccos(dot_pinned(nrm[i], nrm[j]).astype(np.float64)).astype(F32)


def folded_angle(c, angle):
    """the value the threshold is compared with, and the threshold"""
    if c.max_angle >= 0:
        return angle, c.max_angle
    other = F32(np.pi) - angle
    return np.where(other < angle, other, angle), -c.max_angle      # std::min(angle, pi - angle)


def similar(c, i, j, d2):
    """the evaluator's operator() for index arrays i, j and their squared distances"""
    i, j, d2 = np.asarray(i), np.asarray(j), np.asarray(d2, F32)
    ok = np.ones(i.shape, bool)
    if c.max_distance is not None:
        ok &= d2 < c.max_distance
    if c.color_thresh is not None:
        d = c.colors[i] - c.colors[j]
        ok &= dot_pinned(d, d) < c.color_thresh * c.color_thresh
    if c.max_angle is not None:
        v, lim = folded_angle(c, pair_angle(c.normals, i, j))
        with np.errstate(invalid="ignore"):
            ok &= (v <= lim) if c.angle_inclusive else (v < lim)
    return ok


# ---- the literal transcription -----------------------------------------------------------------------------------------------
def brute_lists(p, radius_sq):
    """KDTree::radiusSearch for every point: (index, d2) with d2 < radius_sq, ascending by (d2, index)"""
    p = np.ascontiguousarray(p, F32)
    n = p.shape[0]
    lists = []
    allj = np.arange(n)
    for i in range(n):
        d2 = d2_pinned(p, np.full(n, i), allj)
        with np.errstate(invalid="ignore"):
            hit = np.nonzero(d2 < F32(radius_sq))[0]
        order = np.lexsort((hit, d2[hit]))
        lists.append((hit[order], d2[hit][order]))
    return lists


def serial_reference(lists, n, clauses, seeds=None, min_segment_size=1, max_segment_size=None, skip_first=True):
    """connected_component_extraction.hpp:162-265 line by line over the given lists -> the segments (lists of indices), in the
    reference's order with std::sort made stable"""
    UNASSIGNED = -1
    seeds = list(range(n)) if seeds is None else [int(s) for s in seeds]
    max_segment_size = float("inf") if max_segment_size is None else max_segment_size
    current_label = [UNASSIGNED] * n
    merge = [set() for _ in seeds]
    active = [0] * len(seeds)
    for i, seed in enumerate(seeds):
        if current_label[seed] != UNASSIGNED:
            continue
        merge[i].add(i)
        frontier = [seed]
        current_label[seed] = i
        active[i] = 1
        while frontier:
            cur = frontier.pop()
            idx, val = lists[cur]
            start = 1 if skip_first else 0
            if len(idx) > start:
                ok = similar(clauses, np.full(len(idx) - start, cur), idx[start:], val[start:])
            for k in range(start, len(idx)):
                j = int(idx[k])
                lbl = current_label[j]
                if lbl != i and ok[k - start]:
                    if lbl == UNASSIGNED:
                        frontier.append(j)
                        current_label[j] = i
                    else:
                        merge[i].add(lbl)
    for i in range(len(merge)):
        for it in list(merge[i]):
            merge[it].add(i)
    repr_ = [UNASSIGNED] * len(seeds)
    num = 0
    for i in range(len(seeds)):
        if active[i] == 0 or repr_[i] != UNASSIGNED:
            continue
        frontier = [i]
        repr_[i] = num
        while frontier:
            cur = frontier.pop()
            for it in sorted(merge[cur]):
                if repr_[it] == UNASSIGNED:
                    frontier.append(it)
                    repr_[it] = num
        num += 1
    tmp = [[] for _ in range(num)]
    for i in range(n):
        if current_label[i] == UNASSIGNED:
            continue
        ind = repr_[current_label[i]]
        if len(tmp[ind]) <= max_segment_size:      # :250: a segment past the maximum stops growing one member late ...
            tmp[ind].append(i)
    kept = [s for s in tmp if min_segment_size <= len(s) <= max_segment_size]      # ... and is dropped whole here
    kept.sort(key=len, reverse=True)      # (Python's sort is stable)
    return kept


def segments_to_arrays(segments, n, order_ties=False):
    """-> (labels, offsets, members) as the C entry returns them (clustering_base.hpp:7-18).  order_ties: equal sizes by lowest member --
    what the stable sort already gives with all seeds; with a seed subset the reference's order among equal sizes is that of the seed
    list, which the contract does not keep"""
    if order_ties:
        segments = sorted(segments, key=lambda s: (-len(s), s[0]))
    labels = np.full(n, len(segments), np.int64)
    for k, s in enumerate(segments):
        labels[np.asarray(s, np.int64)] = k
    offsets = np.concatenate([[0], np.cumsum([len(s) for s in segments])]).astype(np.int64)
    unl = np.nonzero(labels == len(segments))[0]
    members = np.concatenate([np.asarray(s, np.int64) for s in segments] + [unl]) if n else np.zeros(0, np.int64)
    return labels, offsets, members


# ---- the union-find restatement ----------------------------------------------------------------------------------------------
def neighbor_pairs(p, radius_sq):
    """every pair i > j of finite points with d2_pinned < radius_sq (strict) -> (i, j, d2), by a grid hash of edge >= the radius"""
    p = np.ascontiguousarray(p, F32)
    n = p.shape[0]
    empty = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F32))
    if not (radius_sq > 0) or n < 2:
        return empty
    fin = np.nonzero(np.isfinite(p).all(axis=1))[0]
    if fin.size < 2:
        return empty
    q = p[fin].astype(np.float64)
    h = np.sqrt(float(radius_sq)) * 1.001
    ext = (q.max(axis=0) - q.min(axis=0)).max()
    h = max(h, ext / 1000.0, 1e-30)      # (a radius far below the cloud's spacing must not ask for 10^9 cells per axis)
    cells = np.floor((q - q.min(axis=0)) / h).astype(np.int64) + 1
    dims = cells.max(axis=0) + 2
    key = (cells[:, 0] * dims[1] + cells[:, 1]) * dims[2] + cells[:, 2]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    out_i, out_j = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                nk = key + (dx * dims[1] + dy) * dims[2] + dz
                lo = np.searchsorted(skey, nk, "left")
                cnt = np.searchsorted(skey, nk, "right") - lo
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                a = np.repeat(np.arange(fin.size), cnt)
                within = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                b = order[np.repeat(lo, cnt) + within]
                m = fin[a] > fin[b]
                out_i.append(fin[a[m]])
                out_j.append(fin[b[m]])
    i = np.concatenate(out_i) if out_i else empty[0]
    j = np.concatenate(out_j) if out_j else empty[1]
    d2 = d2_pinned(p, i, j)
    m = d2 < F32(radius_sq)
    return i[m], j[m], d2[m]


def union_find(n, ei, ej):
    """root[i] = the lowest index of i's component (hooking the larger root under the smaller, then full compression, until no edge
    joins two roots)"""
    lab = np.arange(n, dtype=np.int64)
    ei, ej = np.asarray(ei, np.int64), np.asarray(ej, np.int64)
    while True:
        li, lj = lab[ei], lab[ej]
        diff = li != lj
        if not diff.any():
            return lab
        hi, lo = np.maximum(li, lj)[diff], np.minimum(li, lj)[diff]
        np.minimum.at(lab, hi, lo)
        while True:
            nl = lab[lab]
            if np.array_equal(nl, lab):
                break
            lab = nl
        ei, ej = ei[diff], ej[diff]


def finish(n, root, seeds=None, min_segment_size=1, max_segment_size=None):
    """rule 2 from the roots -> (labels, offsets, members)"""
    size = np.bincount(root, minlength=n)
    is_root = root == np.arange(n)
    keep = is_root & (size >= min_segment_size)
    if max_segment_size is not None:
        keep &= size <= max_segment_size
    if seeds is not None:
        seeded = np.zeros(n, bool)
        seeded[root[np.asarray(seeds, np.int64)]] = True
        keep &= seeded
    roots = np.nonzero(keep)[0]
    roots = roots[np.lexsort((roots, -size[roots]))]      # size descending, equal sizes by lowest member
    rank = np.full(n, len(roots), np.int64)
    rank[roots] = np.arange(len(roots))
    labels = rank[root] if n else np.zeros(0, np.int64)
    members = np.argsort(labels, kind="stable").astype(np.int64)
    offsets = np.searchsorted(labels[members], np.arange(len(roots) + 1), "left").astype(np.int64)
    return labels, offsets, members


_PAIRS = {}


def fast_components(p, radius_sq, clauses=None, seeds=None, min_segment_size=1, max_segment_size=None, stats=None):
    clauses = clauses or Clauses()
    n = p.shape[0]
    key = (id(p), float(radius_sq))      # the pair list of a fixture is computed once and shared by every test that needs it
    if key not in _PAIRS or _PAIRS[key][0] is not p:
        if len(_PAIRS) > 8:
            _PAIRS.clear()
        _PAIRS[key] = (p, neighbor_pairs(p, radius_sq))
    i, j, d2 = _PAIRS[key][1]
    ok = similar(clauses, i, j, d2)
    if stats is not None:
        stats["pairs"], stats["edges"] = int(i.size), int(ok.sum())
    return finish(n, union_find(n, i[ok], j[ok]), seeds, min_segment_size, max_segment_size)


def components_from_lists(n, offsets, idx, keep=None, skip_first=True, seeds=None, min_segment_size=1, max_segment_size=None):
    """the lists entry: weak components of the listed edges (entries >= n are no neighbours)"""
    offsets, idx = np.asarray(offsets, np.int64), np.asarray(idx, np.int64)
    src = np.repeat(np.arange(n), np.diff(offsets))
    use = np.ones(idx.size, bool)
    if skip_first:
        first = offsets[:-1][np.diff(offsets) > 0]
        use[first] = False
    if keep is not None:
        use &= np.asarray(keep).astype(bool)
    use &= (idx < n) & (idx != src)
    return finish(n, union_find(n, src[use], idx[use]), seeds, min_segment_size, max_segment_size)


def ulp_distance(a, b):
    """how many f32 values lie between two positive floats"""
    return np.abs(np.asarray(a, F32).view(np.int32).astype(np.int64) - np.asarray(b, F32).view(np.int32).astype(np.int64))


def near_threshold_counts(p, radius_sq, clauses, ulps=4):
    """-> (pairs whose d2 lies within `ulps` of radius_sq, in-radius pairs whose compared angle lies within `ulps` of its threshold,
    in-radius pairs with dot == 1, with dot > 1)"""
    i, j, d2 = neighbor_pairs(p, F32(radius_sq) * F32(1.0001))
    near_r = int((ulp_distance(d2, np.full(d2.shape, radius_sq, F32)) <= ulps).sum())
    inside = d2 < F32(radius_sq)
    i, j = i[inside], j[inside]
    near_a = ones = above = 0
    if clauses is not None and clauses.max_angle is not None:
        dot = dot_pinned(clauses.normals[i], clauses.normals[j])
        ones, above = int((dot == 1).sum()), int((dot > 1).sum())
        v, lim = folded_angle(clauses, pair_angle(clauses.normals, i, j))
        fin = np.isfinite(v) & (v > 0)
        near_a = int((ulp_distance(v[fin], np.full(int(fin.sum()), lim, F32)) <= ulps).sum())
    return near_r, near_a, ones, above


# ---- the fixtures the CPU and GPU tests share (computed once per process) ----------------------------------------------------
_CACHE = {}
RAW_RADIUS = 0.0048      # raw frame_1: mean degree about 32


def raw_frame():
    import os

    if "raw" not in _CACHE:
        f = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_full.npz"))
        _CACHE["raw"] = (np.ascontiguousarray(f["p1"], F32), np.ascontiguousarray(f["n1"], F32))
    return _CACHE["raw"]


def downsampled_frame():
    """frame_1 after gridDownsample(0.005): 15 531 points with normals (tests/_grid_refs.py, which the device downsampler equals bit for
    bit), seeded random colours, and the normals with seeded random signs"""
    if "ds" not in _CACHE:
        from _grid_refs import grid_downsample_ref

        p, n = raw_frame()
        ds = grid_downsample_ref(p, n, None, 0.005, 1, True)
        pts, nrm = np.ascontiguousarray(ds[0], F32), np.ascontiguousarray(ds[1], F32)
        col = np.random.default_rng(11).random(pts.shape, dtype=F32)
        sign = np.where(np.random.default_rng(7).random(nrm.shape[0]) < 0.5, F32(-1.0), F32(1.0))[:, None]
        _CACHE["ds"] = (pts, nrm, col, (nrm * sign).astype(F32))
    return _CACHE["ds"]


def deg(x):
    return F32(x * np.pi / 180.0)


def evaluator_cases(nrm, nrm_flipped, col):
    """the eight evaluator classes of common_pair_evaluators.hpp:84-259 as (name, constructor arguments, Clauses), each class that has an
    angle with a positive threshold on the frame's normals and a negative one on the sign-flipped normals"""
    D, CT = F32(0.0065 * 0.0065), F32(0.3)      # (tight enough on this frame for every clause to change the result)
    out = [("AlwaysTrueEvaluator", (), Clauses()), ("PointsProximityEvaluator", (D,), Clauses(max_distance=D)),
           ("ColorsProximityEvaluator", (col, CT), Clauses(colors=col, color_thresh=CT)),
           ("PointsColorsProximityEvaluator", (col, D, CT), Clauses(colors=col, max_distance=D, color_thresh=CT))]
    for a, nn in ((deg(5.0), nrm), (-deg(5.0), nrm_flipped)):
        out += [("NormalsProximityEvaluator", (nn, a), Clauses(normals=nn, max_angle=a, angle_inclusive=True)),
                ("PointsNormalsProximityEvaluator", (nn, D, a), Clauses(normals=nn, max_distance=D, max_angle=a)),
                ("NormalsColorsProximityEvaluator", (nn, col, a, CT), Clauses(normals=nn, colors=col, max_angle=a, color_thresh=CT)),
                ("PointsNormalsColorsProximityEvaluator", (nn, col, D, a, CT), Clauses(normals=nn, colors=col, max_distance=D, max_angle=a, color_thresh=CT))]
    return out


def chain(n, spacing, radius, gap_at=None, gap=None, seed=3):
    """n points on a line, `spacing` apart (one gap of `gap` after position gap_at), indices shuffled by a seeded permutation
    -> (points, position of every point along the line)"""
    x = np.arange(n, dtype=np.float64) * spacing
    if gap_at is not None:
        x[gap_at + 1:] += gap - spacing
    pos = np.random.default_rng(seed).permutation(n)      # point i sits at position pos[i]
    p = np.zeros((n, 3), F32)
    p[:, 0] = x[pos].astype(F32)
    return p, pos


def chain_roots(p, radius_sq, joined=None):
    """the components of points on a line, exactly: consecutive points along x are joined iff their pinned d2 < radius_sq (and
    `joined`, per consecutive pair in x order, allows it); points further apart are then never joined without them -> root[]"""
    n = p.shape[0]
    order = np.argsort(p[:, 0], kind="stable")
    link = d2_pinned(p, order[1:], order[:-1]) < F32(radius_sq)
    if joined is not None:
        link &= joined
    run = np.concatenate([[0], np.cumsum(~link)])
    low = np.full(int(run[-1]) + 1, n, np.int64)
    np.minimum.at(low, run, order)
    root = np.empty(n, np.int64)
    root[order] = low[run]
    return root
