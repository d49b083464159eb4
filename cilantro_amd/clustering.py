"""Python mirrors of cilantro's KMeans3f (clustering/kmeans.hpp), ConnectedComponentExtraction3f / 2f / Xf
(clustering/connected_component_extraction.hpp; second part of this file), MeanShift3f / MeanShift2f / MeanShiftXf
(clustering/mean_shift.hpp; third part) and SpectralClustering with KMeansXf and the sparse nearest-neighbour graph matrix (clustering/spectral_clustering.hpp; last part) on top
of the C ABI (cilhip_kmeans3f, cilhip_connected_components3f, cilhip_connected_components_nd, cilhip_mean_shift3f, cilhip_mean_shift_nd, cilhip_nn_graph_matrix /
cilhip_spectral_embedding / cilhip_kmeans_nd).

    km = KMeans3f(points)
    km.cluster(initial_centroids, max_iter=100, tol=eps)      # kmeans.hpp:24-30
    km.cluster(num_clusters, ...)                               # :32-53 (random initial centroids)
    km.getClusterCentroids(); km.getPointToClusterIndexMap(); km.getClusterToPointIndicesMap()

`use_kd_tree=True` (kmeans.hpp:86-94, the mode examples/kmeans.cpp uses): a kd-tree over the centroids only accelerates the same
nearest-centroid search, so the device runs the same exhaustive pass -- with the distance rounded as nanoflann's L2 metric rounds
it (((dx*dx)+(dy*dy))+(dz*dz)), so labels equal that branch's wherever the nearest centroid is unique.
"""
import ctypes as C

import numpy as np

from . import _abi, capi
from .kd_tree import RadiusNeighborhoodSpecification      # noqa: F401 (its home; this module's name for it stays)


class KMeans3f:
    def __init__(self, data, device=0):
        self._L = capi.load()
        self._data = data
        self._device = device
        self.cluster_centroids_ = None
        self.point_to_cluster_index_map_ = None
        self.iteration_count_ = 0

    def cluster(self, centroids_or_k, max_iter=100, tol=float(np.finfo(np.float32).eps), use_kd_tree=False, seed=None):
        p, n, mem, keep = _abi.cloud(self._data)
        if np.isscalar(centroids_or_k):
            # kmeans.hpp:32-53 draws distinct random points (std::random_device): same law, numpy generator
            k = max(1, min(int(centroids_or_k), n))
            idx = np.random.default_rng(seed).choice(n, size=k, replace=False)
            host = keep.cpu().numpy() if hasattr(keep, "cpu") else np.asarray(keep)
            cent = np.ascontiguousarray(host[idx], np.float32)
        else:
            cent = np.ascontiguousarray(centroids_or_k, np.float32).reshape(-1, 3).copy()
        labels = np.zeros(n, np.uint32)
        iters = C.c_size_t(0)
        rc = self._L.cilhip_kmeans3f_ex(self._device, p, n, mem, cent.ctypes.data, len(cent), int(max_iter), C.c_float(tol), int(bool(use_kd_tree)),
                                        labels.ctypes.data, C.byref(iters))
        if rc != capi.OK:
            raise capi.CilhipError(rc, "cilhip_kmeans3f failed (no HIP device, k > 2048, or bad arguments)")
        self.cluster_centroids_ = cent
        self.point_to_cluster_index_map_ = labels.astype(np.int64)
        self.iteration_count_ = int(iters.value)
        return self

    def getClusterCentroids(self):
        return self.cluster_centroids_

    def getNumberOfPerformedIterations(self):
        return self.iteration_count_

    def getPointToClusterIndexMap(self):
        return self.point_to_cluster_index_map_

    def getNumberOfClusters(self):
        return 0 if self.cluster_centroids_ is None else len(self.cluster_centroids_)

    def getClusterToPointIndicesMap(self):
        """clustering_base.hpp:22-33: per cluster, ascending point indices"""
        order = np.argsort(self.point_to_cluster_index_map_, kind="stable")
        counts = np.bincount(self.point_to_cluster_index_map_, minlength=self.getNumberOfClusters())
        return np.split(order, np.cumsum(counts)[:-1])


def set_pruning(on=True):
    """the brute-force branch's assignment computed exactly with pruning (default) or exhaustively (cilhip_kmeans_set_pruning; process-wide)"""
    capi.load().cilhip_kmeans_set_pruning(1 if on else 0)


def kmeans_assign(data, centroids, device=0, use_kd_tree=False):
    L = capi.load()
    p, n, mem, keep = _abi.cloud(data)
    cent = np.ascontiguousarray(centroids, np.float32).reshape(-1, 3)
    labels = np.zeros(n, np.uint32)
    rc = L.cilhip_kmeans3f_assign_ex(device, p, n, mem, cent.ctypes.data, len(cent), int(bool(use_kd_tree)), labels.ctypes.data)
    if rc != capi.OK:
        raise capi.CilhipError(rc, "cilhip_kmeans3f_assign failed")
    return labels.astype(np.int64)


# ---- ConnectedComponentExtraction3f (clustering/connected_component_extraction.hpp) -------------------------------------------
# The contract is stated in include/cilantro_hip/c_api.h (cilhip_connected_components3f) and DESIGN.md section 11.  numpy arrays in ->
# numpy arrays out; device tensors in -> device tensors out.  There is no CPU path: without a usable device every entry raises.
SIZE_MAX = (1 << (8 * C.sizeof(C.c_size_t))) - 1


class AlwaysTrueEvaluator:
    """common_pair_evaluators.hpp:87-88: no clause"""

    normals = colors = None
    max_distance = max_angle = color_thresh = None
    angle_inclusive = False


class PointsProximityEvaluator(AlwaysTrueEvaluator):
    """:92-104"""

    def __init__(self, dist_thresh):
        self.max_distance = dist_thresh


class NormalsProximityEvaluator(AlwaysTrueEvaluator):
    """:106-128 -- the one class whose angle test is <= (:119-121)"""

    angle_inclusive = True

    def __init__(self, normals, angle_thresh):
        self.normals, self.max_angle = normals, angle_thresh


class ColorsProximityEvaluator(AlwaysTrueEvaluator):
    """:130-146"""

    def __init__(self, colors, dist_thresh):
        self.colors, self.color_thresh = colors, dist_thresh


class PointsNormalsProximityEvaluator(AlwaysTrueEvaluator):
    """:148-172"""

    def __init__(self, normals, dist_thresh, angle_thresh):
        self.normals, self.max_distance, self.max_angle = normals, dist_thresh, angle_thresh


class PointsColorsProximityEvaluator(AlwaysTrueEvaluator):
    """:174-193"""

    def __init__(self, colors, dist_thresh, color_thresh):
        self.colors, self.max_distance, self.color_thresh = colors, dist_thresh, color_thresh


class NormalsColorsProximityEvaluator(AlwaysTrueEvaluator):
    """:195-224"""

    def __init__(self, normals, colors, angle_thresh, color_thresh):
        self.normals, self.colors, self.max_angle, self.color_thresh = normals, colors, angle_thresh, color_thresh


class PointsNormalsColorsProximityEvaluator(AlwaysTrueEvaluator):
    """:226-259"""

    def __init__(self, normals, colors, dist_thresh, angle_thresh, color_thresh):
        self.normals, self.colors, self.max_distance, self.max_angle, self.color_thresh = normals, colors, dist_thresh, angle_thresh, color_thresh


def _cc_seeds(seeds):
    """-> (pointer or None, count, keepalive): the seed list is always a host array"""
    if seeds is None:
        return None, 0, None
    if hasattr(seeds, "cpu"):
        seeds = seeds.cpu().numpy()
    s = np.asarray(seeds)
    if s.size and (s.min() < 0 or s.max() > 0xFFFFFFFF):
        raise ValueError("seed indices must lie in [0, n)")
    s = np.ascontiguousarray(s, np.uint32).reshape(-1)
    keep = s if s.size else np.zeros(1, np.uint32)      # (an empty list is still a list: a non-null pointer)
    return keep.ctypes.data, s.size, keep


def _segments(labels, offsets, members, nseg):
    """-> (labels, offsets[nseg + 1], members[n]) as int64"""
    return _abi.widen(labels), _abi.widen(offsets[: nseg + 1]), _abi.widen(members)


def _cloud(a, what):
    return _abi.rows(a, 3, "clouds", none_ok=True)


def _nd_rows(a, what):
    return _abi.rows(a, None, what, cast=True)


def _connected_components(nd, points, radius_sq, evaluator, min_segment_size, max_segment_size, seeds, device, form=0, stats=None):
    """the one body of connected_components() (N x 3 clouds, float32 or TypeError) and connected_components_nd() (n x dim, converted)"""
    L = capi.load()
    ev = evaluator if evaluator is not None else AlwaysTrueEvaluator()
    take = _nd_rows if nd else _cloud
    x = take(points, "the points")
    ptrs, keep = [None, None], [x.keep]
    for k, (att, width, what) in enumerate(((ev.normals, x.dim, "the normals"), (ev.colors, 3, "the colours"))):
        if att is None:
            continue
        a = take(att, what)
        if a.n != x.n or (nd and a.dim != width):
            raise ValueError("the normals are an n x dim array and the colours an n x 3 array over the points' n" if nd else
                             "points, normals and colors must have the same number of rows")
        if a.mem != x.mem:
            raise ValueError("points, normals and colors must live in the same memory space")
        ptrs[k] = a.ptr
        keep.append(a.keep)
    prm = capi.CcParams()
    L.cilhip_cc_default_params(C.byref(prm))
    prm.radius_sq = radius_sq
    if ev.max_distance is not None:
        prm.use_distance, prm.max_distance = 1, ev.max_distance
    if ev.max_angle is not None:
        prm.use_normals, prm.max_angle, prm.angle_inclusive = 1, ev.max_angle, int(ev.angle_inclusive)
    if ev.color_thresh is not None:
        prm.use_colors, prm.color_thresh = 1, ev.color_thresh
    prm.min_segment_size, prm.max_segment_size = int(min_segment_size), min(int(max_segment_size), SIZE_MAX)
    sp, ns, skeep = _cc_seeds(seeds)
    n = x.n
    device, dev = _abi.enter(x.keep, device)
    outs = [_abi.empty(m, np.uint32, dev) for m in (n, n + 1, n)]
    addr = [_abi.ptr(o) for o in outs]
    nseg = C.c_size_t(0)
    if nd:
        rc = L.cilhip_connected_components_nd(device, x.ptr if n else None, ptrs[0], ptrs[1], n, x.dim, x.mem, C.byref(prm), int(form), sp, ns, *addr, C.byref(nseg))
    else:
        rc = L.cilhip_connected_components3f(device, x.ptr, ptrs[0], ptrs[1], n, x.mem, C.byref(prm), sp, ns, *addr, C.byref(nseg))
    _abi.check(rc, "cilhip_connected_components_nd" if nd else "cilhip_connected_components3f", L)
    if n == 0:
        outs[1][:1] = 0
    elif nd and stats is not None:
        st = capi.CcnStats()
        L.cilhip_ccn_last_stats(C.byref(st))
        stats.update({k: getattr(st, k) for k, _ in capi.CcnStats._fields_})
    return _segments(*outs, nseg.value)


def connected_components(points, radius_sq, evaluator=None, min_segment_size=1, max_segment_size=SIZE_MAX, seeds=None, device=0):
    """cilhip_connected_components3f -> (labels[n], offsets[segments + 1], members[n]): segment k is members[offsets[k]:offsets[k + 1]],
    members[offsets[-1]:] are the unlabelled points; labels[i] == segments for those"""
    return _connected_components(False, points, radius_sq, evaluator, min_segment_size, max_segment_size, seeds, device)


def connected_components_from_lists(n, offsets, idx, keep=None, skip_first=True, symmetric=True, min_segment_size=1, max_segment_size=SIZE_MAX, seeds=None,
                                    device=0):
    """cilhip_connected_components_lists: the reference's "given neighbours" overloads (:20-160) over CSR lists -- of cilhip_radius_search3f
    (symmetric) or cilhip_knn3f (directed: weak components; offsets = arange(n + 1) * k) -- with an optional byte mask per entry"""
    L = capi.load()
    if _abi.on_device(idx):
        import torch

        off = offsets.to(device=idx.device, dtype=torch.int64).contiguous()
        ix = idx.to(torch.int32).contiguous() if idx.dtype != torch.int32 else idx.contiguous()
        kp = None if keep is None else keep.to(device=idx.device, dtype=torch.uint8).contiguous()
        total, mem = ix.numel(), capi.MEM_DEVICE
    else:
        off = np.ascontiguousarray(offsets, np.uint64)
        ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        kp = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
        total, mem = ix.size, capi.MEM_HOST
    device, dev = _abi.enter(ix, device)
    if len(off) != n + 1 or (kp is not None and len(kp) != total):
        raise ValueError("offsets must have n + 1 entries and keep one byte per list entry")
    sp, ns, skeep = _cc_seeds(seeds)
    outs = [_abi.empty(m, np.uint32, dev) for m in (n, n + 1, n)]
    nseg = C.c_size_t(0)
    rc = L.cilhip_connected_components_lists(device, n, _abi.ptr(off), _abi.ptr(ix), _abi.ptr(kp), total, int(bool(skip_first)), int(bool(symmetric)), mem,
                                             int(min_segment_size), min(int(max_segment_size), SIZE_MAX), sp, ns, *[_abi.ptr(o) for o in outs], C.byref(nseg))
    _abi.check(rc, "cilhip_connected_components_lists", L)
    if n == 0:
        outs[1][:1] = 0
    return _segments(*outs, nseg.value)


class ConnectedComponentExtraction3f:
    """connected_component_extraction.hpp:368-428 with the ClusteringBase accessors (clustering_base.hpp:60-97)

        cce = ConnectedComponentExtraction3f(points)
        cce.segment(RadiusNeighborhoodSpecification(0.02 ** 2), NormalsProximityEvaluator(normals, np.radians(2)), 100, n)
        cce.segment(nh, seeds, evaluator, min_segment_size, max_segment_size)      # :394-407
    Other neighbourhood kinds and user functors: connected_components_from_lists()."""

    def __init__(self, points, device=0):
        self._points = points
        self._device = device
        self._labels = self._offsets = self._members = None

    def segment(self, nh, *args, **kw):
        if not isinstance(nh, RadiusNeighborhoodSpecification):
            raise TypeError("segment() takes a RadiusNeighborhoodSpecification (other neighbourhoods: connected_components_from_lists)")
        args = list(args)
        seeds = kw.pop("seeds", None)
        if args and args[0] is not None and not isinstance(args[0], AlwaysTrueEvaluator):
            seeds = args.pop(0)      # segment(nh, seeds_ind, evaluator, min, max)
        for k, v in zip(("evaluator", "min_segment_size", "max_segment_size"), args):
            kw[k] = v
        self._labels, self._offsets, self._members = self._components(nh.radius, kw.get("evaluator"), kw.get("min_segment_size", 1), kw.get("max_segment_size", SIZE_MAX), seeds)
        return self

    def _components(self, radius_sq, evaluator, min_segment_size, max_segment_size, seeds):
        return connected_components(self._points, radius_sq, evaluator, min_segment_size, max_segment_size, seeds, self._device)

    def getPointToClusterIndexMap(self):
        return self._labels

    def getNumberOfClusters(self):
        return 0 if self._offsets is None else int(self._offsets.shape[0]) - 1

    def getNumberOfPoints(self):
        return 0 if self._labels is None else int(self._labels.shape[0])

    def getClusterToPointIndicesMap(self):
        """per cluster, ascending point indices"""
        k = self.getNumberOfClusters()
        return [self._members[int(self._offsets[c]):int(self._offsets[c + 1])] for c in range(k)]

    def getLabeledPointIndices(self):
        return (self._labels < self.getNumberOfClusters()).nonzero()[0] if isinstance(self._labels, np.ndarray) else (self._labels < self.getNumberOfClusters()).nonzero().reshape(-1)

    def getUnlabeledPointIndices(self):
        return self._members[int(self._offsets[-1]):]


# ---- ConnectedComponentExtractionXf / 2f (connected_component_extraction.hpp:162-265, :394-457 for EigenDim 2 and Dynamic) -----------
# The contract is stated in include/cilantro_hip/c_api.h (cilhip_connected_components_nd, rules C1-C5) and DESIGN.md section 23.
def connected_components_nd(points, radius_sq, evaluator=None, min_segment_size=1, max_segment_size=SIZE_MAX, seeds=None, form=0, device=0, stats=None):
    """cilhip_connected_components_nd over n x dim points (1 <= dim <= 16) -> (labels[n], offsets[segments + 1], members[n]) as
    connected_components() returns them.  The evaluator's normals are n x dim, its colours n x 3.  form: 0 the code decides, 1 the
    exhaustive triangle, 2 sweep and prune (the same words, rule C4).  stats: a dict that receives cilhip_ccn_last_stats.  numpy arrays
    in -> numpy arrays out; device tensors in -> device tensors out"""
    return _connected_components(True, points, radius_sq, evaluator, min_segment_size, max_segment_size, seeds, device, form, stats)


class ConnectedComponentExtractionXf(ConnectedComponentExtraction3f):
    """ConnectedComponentExtraction<float, Dynamic> (connected_component_extraction.hpp:368-457): ConnectedComponentExtraction3f's
    segment() forms and accessors over n x dim points, 1 <= dim <= 16.  dim, when given, is checked against the points.  form: see
    connected_components_nd(); getLastStats(): what the last segment() did (cilhip_ccn_stats)."""

    def __init__(self, points, dim=None, device=0, form=0):
        super().__init__(points, device)
        if getattr(points, "ndim", None) != 2 or (dim is not None and int(points.shape[1]) != int(dim)):
            raise ValueError("the points are an n x dim array" if dim is None else f"the points are an n x {int(dim)} array")
        self.dim = int(points.shape[1])
        self._form = form
        self._stats = {}

    def _components(self, radius_sq, evaluator, min_segment_size, max_segment_size, seeds):
        self._stats = {}
        return connected_components_nd(self._points, radius_sq, evaluator, min_segment_size, max_segment_size, seeds, self._form, self._device, self._stats)

    def getLastStats(self):
        return dict(self._stats)


class ConnectedComponentExtraction2f(ConnectedComponentExtractionXf):
    """ConnectedComponentExtraction<float, 2>"""

    def __init__(self, points, device=0, form=0):
        super().__init__(points, 2, device, form)


# ---- MeanShift3f (clustering/mean_shift.hpp) ------------------------------------------------------------------------------------
# The contract is stated in include/cilantro_hip/c_api.h (cilhip_mean_shift3f) and DESIGN.md section 13.  numpy arrays in -> numpy arrays
# out; device tensors in -> device tensors out.  There is no CPU path.
class UnityWeightEvaluator:
    """common_pair_evaluators.hpp:30-43"""

    kind, sigma = 0, 1.0


class IdentityWeightEvaluator(UnityWeightEvaluator):
    """:14-27 -- the weight is the squared distance"""

    kind = 1


class RBFKernelWeightEvaluator(UnityWeightEvaluator):
    """:46-80 -- exp(-0.5 / sigma^2 * squared distance)"""

    kind = 2

    def __init__(self, sigma=1.0):
        self.sigma = float(sigma)


_MS_STATS = (("form_used", "est_ball", "shift_ms", "group_ms", "passes", "rounds"), ("passes", "rounds", "slices_first", "slices_last", "shift_ms", "group_ms"))


def _mean_shift(nd, points, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator, seeds, device, form=None):
    """the one body of mean_shift() (N x 3 clouds, float32 or TypeError) and mean_shift_nd() (n x dim, converted)"""
    L = capi.load()
    ev = evaluator if evaluator is not None else UnityWeightEvaluator()
    take = _nd_rows if nd else _cloud
    x = take(points, "the points")
    n, dim = x.n, (x.dim if nd else 3)
    sp, ns, keep_s = None, n, None
    if seeds is not None:
        s = take(seeds, "the seeds")
        sp, ns, keep_s = s.ptr, s.n, s.keep
        if s.mem != x.mem:
            raise ValueError("points and seeds must live in the same memory space")
        if s.dim != dim:
            raise ValueError("points and seeds must have the same dimension")
        if ns == 0:      # (an empty list is still a list: a non-null pointer)
            keep_s = _abi.empty((1, max(dim, 1)), np.float32, x.keep.device if x.mem == capi.MEM_DEVICE else None, zero=True)
            sp = _abi.ptr(keep_s)
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol, prm.convergence_tol = kernel_radius, int(max_iter), cluster_tol, convergence_tol
    prm.kernel_kind, prm.kernel_sigma = int(ev.kind), float(ev.sigma)
    if form is not None:
        prm.form = int(form)
    device, dev = _abi.enter(x.keep, device)
    shifted, modes = _abi.empty((ns, dim), np.float32, dev), _abi.empty((ns, dim), np.float32, dev)
    labels, offsets, members = (_abi.empty(m, np.uint32, dev) for m in (ns, ns + 1, ns))
    nc, iters = C.c_size_t(0), C.c_size_t(0)
    outs = [_abi.ptr(o) for o in (shifted, labels, modes, offsets, members)] + [C.byref(nc), C.byref(iters)]
    n_seeds = ns if seeds is not None else 0
    if nd:
        rc = L.cilhip_mean_shift_nd(device, x.ptr, n, dim, sp, n_seeds, x.mem, C.byref(prm), *outs)
    else:
        rc = L.cilhip_mean_shift3f(device, x.ptr, n, sp, n_seeds, x.mem, C.byref(prm), *outs)
    _abi.check(rc, "cilhip_mean_shift_nd" if nd else "cilhip_mean_shift3f", L)
    if ns == 0:
        offsets[:1] = 0
    st = capi.MsnStats() if nd else capi.MsStats()
    (L.cilhip_msn_last_stats if nd else L.cilhip_ms_last_stats)(C.byref(st))
    stats = {k: getattr(st, k) for k in _MS_STATS[nd]} if ns else {}
    lab, off, mem_ = _segments(labels, offsets, members, nc.value)
    return {"shifted": shifted, "labels": lab, "modes": modes[: nc.value], "offsets": off, "members": mem_, "iterations": int(iters.value), "stats": stats}


def mean_shift(points, kernel_radius, max_iter, cluster_tol, convergence_tol=float(np.finfo(np.float32).eps), evaluator=None, seeds=None, form=0, device=0):
    """cilhip_mean_shift3f -> dict(shifted[ns, 3], labels[ns], modes[k, 3], offsets[k + 1], members[ns], iterations, stats): cluster c is
    members[offsets[c]:offsets[c + 1]]; seeds=None: every point is a seed"""
    return _mean_shift(False, points, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator, seeds, device, form)


class MeanShift3f:
    """mean_shift.hpp:12-140 with the ClusteringBase accessors (clustering_base.hpp:60-97)

        ms = MeanShift3f(points)
        ms.cluster(2.0, 5000, 0.2, 1e-7, UnityWeightEvaluator())               # :118-124 -- every point is a seed
        ms.cluster(seeds, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator)      # :38-115
    A tree handed to the reference's second constructor is "the same points" here."""

    def __init__(self, points, device=0):
        self._points = points
        self._device = device
        self._r = None

    def cluster(self, *args, **kw):
        args = list(args)
        seeds = kw.pop("seeds", None)
        if args and not np.isscalar(args[0]):
            seeds = args.pop(0)
        for k, v in zip(("kernel_radius", "max_iter", "cluster_tol", "convergence_tol", "evaluator"), args):
            kw[k] = v
        self._r = self._mean_shift(self._points, seeds=seeds, device=self._device, **kw)
        return self

    _mean_shift = staticmethod(mean_shift)

    def getShiftedSeeds(self):
        return self._r["shifted"]

    def getClusterModes(self):
        return self._r["modes"]

    def getNumberOfPerformedIterations(self):
        return self._r["iterations"]

    def getPointToClusterIndexMap(self):
        return self._r["labels"]

    def getNumberOfClusters(self):
        return int(self._r["offsets"].shape[0]) - 1

    def getClusterToPointIndicesMap(self):
        """per cluster, ascending seed indices"""
        off, mem = self._r["offsets"], self._r["members"]
        return [mem[int(off[c]):int(off[c + 1])] for c in range(self.getNumberOfClusters())]


# ---- MeanShiftXf / MeanShift2f (clustering/mean_shift.hpp:142-164) -----------------------------------------------------------------
# The contract is stated in include/cilantro_hip/c_api.h (cilhip_mean_shift_nd, rules M1-M7) and DESIGN.md section 22.
def mean_shift_nd(points, kernel_radius, max_iter, cluster_tol, convergence_tol=float(np.finfo(np.float32).eps), evaluator=None, seeds=None, device=0):
    """cilhip_mean_shift_nd over n x dim points (1 <= dim <= 16) -> dict(shifted[ns, dim], labels[ns], modes[k, dim], offsets[k + 1],
    members[ns], iterations, stats): cluster c is members[offsets[c]:offsets[c + 1]]; seeds=None: every point is a seed.  numpy arrays in ->
    numpy arrays out; device tensors in -> device tensors out"""
    return _mean_shift(True, points, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator, seeds, device)


class MeanShiftXf(MeanShift3f):
    """MeanShift<float, Dynamic> (mean_shift.hpp:164): MeanShift3f's two cluster() forms and accessors over n x dim points, 1 <= dim <= 16.
    dim, when given, is checked against the points."""

    def __init__(self, points, dim=None, device=0):
        super().__init__(points, device)
        if getattr(points, "ndim", None) != 2 or (dim is not None and int(points.shape[1]) != int(dim)):
            raise ValueError("the points are an n x dim array" if dim is None else f"the points are an n x {int(dim)} array")
        self.dim = int(points.shape[1])

    _mean_shift = staticmethod(mean_shift_nd)


class MeanShift2f(MeanShiftXf):
    """MeanShift<float, 2> (mean_shift.hpp:142)"""

    def __init__(self, points, device=0):
        super().__init__(points, 2, device)


# ---- SpectralClustering (clustering/spectral_clustering.hpp) ---------------------------------------------------------------------
# The contract is stated in include/cilantro_hip/c_api.h (rules S1-S6) and DESIGN.md section 18.  There is no CPU path.
class GraphLaplacianType:
    """spectral_clustering.hpp:44"""

    UNNORMALIZED, NORMALIZED_SYMMETRIC, NORMALIZED_RANDOM_WALK = 0, 1, 2


class SparseMatrix:
    """owner of a cilhip_sparse handle (a CSR matrix on the device); close() or the garbage collector frees it"""

    def __init__(self, handle, device):
        self._L, self._h, self.device = capi.load(), handle, device

    @classmethod
    def from_csr(cls, n, offsets, columns, values, device=0):
        """cilhip_sparse_from_csr: numpy arrays, or device tensors (int64 offsets, int32 columns, float32 values)"""
        L = capi.load()
        if _abi.on_device(values):
            import torch

            off, col, val = offsets.to(torch.int64).contiguous(), columns.to(torch.int32).contiguous(), values.to(torch.float32).contiguous()
            mem = capi.MEM_DEVICE
        else:
            off, col, val = np.ascontiguousarray(offsets, np.uint64), np.ascontiguousarray(columns, np.uint32), np.ascontiguousarray(values, np.float32)
            col, val = (col if col.size else np.zeros(1, np.uint32)), (val if val.size else np.zeros(1, np.float32))
            mem = capi.MEM_HOST
        device, _ = _abi.enter(val, device)
        if len(off) != n + 1:
            raise ValueError("offsets must have n + 1 entries")
        h = C.c_void_p()
        _abi.check(L.cilhip_sparse_from_csr(device, int(n), _abi.ptr(off), _abi.ptr(col), _abi.ptr(val), mem, C.byref(h)), "cilhip_sparse_from_csr", L)
        return cls(h, device)

    @classmethod
    def from_dense(cls, dense, device=0):
        """a dense affinity matrix, converted to CSR on the host (the entries that are not zero)"""
        a = np.asarray(dense.cpu() if hasattr(dense, "cpu") else dense, np.float32)
        if a.ndim != 2 or a.shape[0] != a.shape[1]:
            raise ValueError("a dense affinity matrix is square")
        rows, cols = np.nonzero(a)
        off = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=a.shape[0])))).astype(np.uint64)
        return cls.from_csr(a.shape[0], off, cols.astype(np.uint32), a[rows, cols], device)

    def info(self):
        """-> (n, nnz, longest row)"""
        v = [C.c_size_t(0) for _ in range(3)]
        self._L.cilhip_sparse_info(self._h, *[C.byref(x) for x in v])
        return tuple(int(x.value) for x in v)

    def get(self, on_device=False):
        """cilhip_sparse_get -> (offsets[n + 1], columns[nnz], values[nnz]): numpy (uint64, uint32, float32) or device tensors (int64, int32, float32)"""
        n, nnz, _ = self.info()
        dev = f"cuda:{self.device}" if on_device else None
        out = [_abi.empty(n + 1, np.uint64, dev), _abi.empty(max(nnz, 1), np.uint32, dev), _abi.empty(max(nnz, 1), np.float32, dev)]
        _abi.enter(out[0], self.device)
        rc = self._L.cilhip_sparse_get(self._h, _abi.ptr(out[0]), _abi.ptr(out[1]), _abi.ptr(out[2]), capi.MEM_DEVICE if on_device else capi.MEM_HOST)
        _abi.check(rc, "cilhip_sparse_get", self._L)
        return out[0], out[1][:nnz], out[2][:nnz]

    def close(self):
        if self._h:
            self._L.cilhip_sparse_destroy(self._h)
            self._h = None

    __del__ = close


def nn_graph_sparse_matrix(neighbors, evaluator=None, force_symmetry=False, duplicates=0, device=0):
    """getNNGraphFunctionValueSparseMatrix (nearest_neighbor_graph_utilities.hpp:89-118; duplicates=1: the dense variant's assignment rule,
    :63-87) -> SparseMatrix.  neighbors: (idx[n, k], d2[n, k]) as KDTree3f.kNNSearch returns them (-1 or 0xFFFFFFFF pads a short list) or
    (offsets[n + 1], idx, d2) as radiusSearch does; numpy arrays or device tensors.  The first entry of a list, the point itself, is kept."""
    L = capi.load()
    ev = evaluator if evaluator is not None else UnityWeightEvaluator()
    offsets = None
    if len(neighbors) == 3 and np.ndim(neighbors[1]) == 1:
        offsets, idx, d2 = neighbors
    else:
        idx, d2 = neighbors[0], neighbors[1]
    on_device = _abi.on_device(idx)
    if on_device:
        import torch

        ix = idx.to(torch.int32).contiguous()
        dd = None if d2 is None else d2.to(device=idx.device, dtype=torch.float32).contiguous()
        off = None if offsets is None else offsets.to(device=idx.device, dtype=torch.int64).contiguous()
        shape, mem = tuple(ix.shape), capi.MEM_DEVICE
    else:
        ix = np.ascontiguousarray(np.asarray(idx).astype(np.int64) & 0xFFFFFFFF, np.uint32)
        dd = None if d2 is None else np.ascontiguousarray(d2, np.float32)
        off = None if offsets is None else np.ascontiguousarray(offsets, np.uint64)
        shape, mem = ix.shape, capi.MEM_HOST
    device, _ = _abi.enter(ix, device)
    if off is None:
        if len(shape) != 2:
            raise ValueError("a k-NN list is an n x k array")
        n, k_or_total = int(shape[0]), int(shape[1])
    else:
        n, k_or_total = len(off) - 1, int(np.prod(shape))
        if not on_device and ix.size == 0:
            ix, dd = np.zeros(1, np.uint32), (None if dd is None else np.zeros(1, np.float32))
    h = C.c_void_p()
    rc = L.cilhip_nn_graph_matrix(device, n, _abi.ptr(off), _abi.ptr(ix), _abi.ptr(dd), k_or_total, mem, int(ev.kind), C.c_float(ev.sigma), int(bool(force_symmetry)), int(duplicates),
                                  C.byref(h))
    _abi.check(rc, "cilhip_nn_graph_matrix", L)
    return SparseMatrix(h, device)


def spectral_embedding(affinities, max_num_clusters, estimate_num_clusters=False, laplacian_type=GraphLaplacianType.NORMALIZED_RANDOM_WALK, on_device=False, max_outer=None,
                       degree=None, guard=None, raise_unconverged=True):
    """cilhip_spectral_embedding -> (embedded[n, num_clusters] f32, eigenvalues[nev] f32, result dict).  Raises when the solver gave up
    (n_converged < num_eigenvalues after max_outer iterations) unless raise_unconverged is False."""
    L = capi.load()
    n = affinities.info()[0]
    prm = capi.SpectralParams()
    L.cilhip_spectral_default_params(C.byref(prm))
    prm.max_num_clusters, prm.estimate_num_clusters, prm.laplacian_type = int(max_num_clusters), int(bool(estimate_num_clusters)), int(laplacian_type)
    for key, v in (("max_outer", max_outer), ("degree", degree), ("guard", guard)):
        if v is not None:
            setattr(prm, key, int(v))
    room = max(min(int(max_num_clusters), 16), 2)
    emb = _abi.empty((n, room), np.float32, f"cuda:{affinities.device}" if on_device else None)
    _abi.enter(emb, affinities.device)
    ev = np.zeros(room + 1, np.float32)
    res = capi.SpectralResult()
    rc = L.cilhip_spectral_embedding(affinities._h, C.byref(prm), _abi.ptr(emb), ev.ctypes.data, capi.MEM_DEVICE if on_device else capi.MEM_HOST, C.byref(res))
    _abi.check(rc, "cilhip_spectral_embedding", L)
    info = {k: getattr(res, k) for k, _ in capi.SpectralResult._fields_}
    if raise_unconverged and res.n_converged < res.num_eigenvalues:
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "cilhip_spectral_embedding: %d of %d eigenpairs converged in %d outer iterations (largest residual %.3g)"
                               % (res.n_converged, res.num_eigenvalues, res.outer_iterations, res.max_residual))
    nc = int(res.num_clusters)
    flat = emb.reshape(-1)[: n * nc]      # (point-major n x num_clusters at the start of the buffer)
    return flat.reshape(n, nc), ev[: res.num_eigenvalues].copy(), info


class KMeansXf(KMeans3f):
    """KMeans<float, Dynamic> (kmeans.hpp:67-194), brute-force branch, 1 <= dim <= 16 (cilhip_kmeans_nd, rule S6).  data: n x dim, a numpy
    array or a device tensor.  use_kd_tree is accepted and changes nothing: the kd-tree branch is not built in D dimensions."""

    def cluster(self, centroids_or_k, max_iter=100, tol=float(np.finfo(np.float32).eps), use_kd_tree=False, seed=None):
        r = _nd_rows(self._data, "the points")
        x, n, dim = r.keep, r.n, r.dim
        device, dev = _abi.enter(x, self._device)
        if np.isscalar(centroids_or_k):
            k = max(1, min(int(centroids_or_k), n))
            idx = np.sort(np.random.default_rng(seed).choice(n, size=k, replace=False))
            if dev is not None:
                import torch

                idx = torch.as_tensor(idx, device=dev)
            cent = np.ascontiguousarray(x[idx].cpu().numpy() if dev is not None else x[idx], np.float32)
        else:
            cent = np.ascontiguousarray(centroids_or_k.cpu() if hasattr(centroids_or_k, "cpu") else centroids_or_k, np.float32).reshape(-1, dim).copy()
        labels = _abi.empty(n, np.uint32, dev, zero=True)
        _abi.enter(labels, device)      # (the zeros are torch's work too)
        iters = C.c_size_t(0)
        rc = self._L.cilhip_kmeans_nd(device, r.ptr, n, dim, r.mem, cent.ctypes.data, len(cent), int(max_iter), C.c_float(tol), _abi.ptr(labels), C.byref(iters))
        _abi.check(rc, "cilhip_kmeans_nd", self._L)
        self.cluster_centroids_ = cent
        self.point_to_cluster_index_map_ = (labels.cpu().numpy() if dev is not None else labels).astype(np.int64)
        self.iteration_count_ = int(iters.value)
        return self


class SpectralClustering(KMeansXf):
    """SpectralClustering<float, Dynamic> (spectral_clustering.hpp:316-416): the Laplacian embedding of an affinity matrix, then k-means
    on the embedded points with num_clusters centroids.

        sc = SpectralClustering(affinities, 4, True, GraphLaplacianType.NORMALIZED_RANDOM_WALK)
    affinities: a SparseMatrix (nn_graph_sparse_matrix), a CSR triple (offsets, columns, values) or a dense square array (converted to CSR
    on the host).  The reference starts k-means from random points (std::random_device): `seed` seeds that draw, or
    initial_centroid_indices names the points.  kmeans_use_kd_tree is accepted and changes nothing (KMeansXf)."""

    def __init__(self, affinities, max_num_clusters, estimate_num_clusters=False, laplacian_type=GraphLaplacianType.NORMALIZED_RANDOM_WALK, kmeans_max_iter=100,
                 kmeans_conv_tol=float(np.finfo(np.float32).eps), kmeans_use_kd_tree=False, seed=None, initial_centroid_indices=None, device=0):
        own = not isinstance(affinities, SparseMatrix)
        if own:
            if isinstance(affinities, (tuple, list)) and len(affinities) == 3:
                affinities = SparseMatrix.from_csr(len(affinities[0]) - 1, affinities[0], affinities[1], affinities[2], device)
            else:
                affinities = SparseMatrix.from_dense(affinities, device)
        try:
            self.embedded_points_, self.computed_eigenvalues_, self.embedding_info_ = spectral_embedding(affinities, max_num_clusters, estimate_num_clusters, laplacian_type)
        finally:
            if own:
                affinities.close()
        super().__init__(self.embedded_points_, affinities.device)
        k = self.embedded_points_.shape[1]
        if initial_centroid_indices is not None:
            start = self.embedded_points_[np.asarray(initial_centroid_indices, np.int64)[:k]]
        else:
            start = k
        self.cluster(start, kmeans_max_iter, kmeans_conv_tol, kmeans_use_kd_tree, seed)

    def getEmbeddedPoints(self):
        """n x num_clusters (the reference's dim x n, column-major: the same bytes)"""
        return self.embedded_points_

    def getComputedEigenValues(self):
        return self.computed_eigenvalues_

    def getEmbeddingDimension(self):
        return int(self.embedded_points_.shape[1])
