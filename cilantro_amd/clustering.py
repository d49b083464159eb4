"""Python mirrors of cilantro's KMeans3f (clustering/kmeans.hpp), ConnectedComponentExtraction3f
(clustering/connected_component_extraction.hpp; second part of this file) and MeanShift3f (clustering/mean_shift.hpp; last part) on top
of the C ABI (cilhip_kmeans3f, cilhip_connected_components3f, cilhip_mean_shift3f).

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

from . import capi
from .icp import _as_cloud


class KMeans3f:
    def __init__(self, data, device=0):
        self._L = capi.load()
        self._data = data
        self._device = device
        self.cluster_centroids_ = None
        self.point_to_cluster_index_map_ = None
        self.iteration_count_ = 0

    def cluster(self, centroids_or_k, max_iter=100, tol=float(np.finfo(np.float32).eps), use_kd_tree=False, seed=None):
        p, n, mem, keep = _as_cloud(self._data)
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
    p, n, mem, keep = _as_cloud(data)
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


class RadiusNeighborhoodSpecification:
    """core/nearest_neighbors.hpp: the radius is the SQUARED distance, as in the reference"""

    def __init__(self, radius_sq):
        self.radius = float(radius_sq)


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


def _cc_outputs(n, on_device, dev):
    if on_device:
        import torch

        outs = [torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n + 1, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)]
        return outs, [o.data_ptr() for o in outs]
    outs = [np.empty(n, np.uint32), np.empty(n + 1, np.uint32), np.empty(n, np.uint32)]
    return outs, [o.ctypes.data for o in outs]


def _cc_result(outs, nseg, on_device):
    """-> (labels, offsets[nseg + 1], members[n]) as int64"""
    labels, offsets, members = outs
    if on_device:
        import torch

        # (uint32 words in int32 tensors: widen without the sign)
        wide = lambda t: t.to(torch.int64) & 0xFFFFFFFF      # noqa: E731
        return wide(labels), wide(offsets[: nseg + 1]), wide(members)
    return labels.astype(np.int64), offsets[: nseg + 1].astype(np.int64), members.astype(np.int64)


def connected_components(points, radius_sq, evaluator=None, min_segment_size=1, max_segment_size=SIZE_MAX, seeds=None, device=0):
    """cilhip_connected_components3f -> (labels[n], offsets[segments + 1], members[n]): segment k is members[offsets[k]:offsets[k + 1]],
    members[offsets[-1]:] are the unlabelled points; labels[i] == segments for those"""
    L = capi.load()
    ev = evaluator if evaluator is not None else AlwaysTrueEvaluator()
    p, n, mem, keep_p = _as_cloud(points)
    ptrs, keep = [None, None], [keep_p]
    for k, att in enumerate((ev.normals, ev.colors)):
        if att is None:
            continue
        ap, an, amem, akeep = _as_cloud(att)
        if an != n:
            raise ValueError("points, normals and colors must have the same number of rows")
        if amem != mem:
            raise ValueError("points, normals and colors must live in the same memory space")
        ptrs[k] = ap
        keep.append(akeep)
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
    on_device = mem == capi.MEM_DEVICE
    dev = None
    if on_device:
        import torch

        dev = keep_p.device
        if dev.index is not None:
            device = dev.index
        torch.cuda.synchronize(dev)      # the call runs on a stream of its own: the inputs must be complete
    outs, addr = _cc_outputs(n, on_device, dev)
    nseg = C.c_size_t(0)
    rc = L.cilhip_connected_components3f(int(device), p, ptrs[0], ptrs[1], n, mem, C.byref(prm), sp, ns, addr[0], addr[1], addr[2], C.byref(nseg))
    if rc != capi.OK:
        raise capi.CilhipError(rc, "cilhip_connected_components3f: " + L.cilhip_last_error(None).decode())
    if n == 0:
        outs[1][:1] = 0
    return _cc_result(outs, nseg.value, on_device)


def connected_components_from_lists(n, offsets, idx, keep=None, skip_first=True, symmetric=True, min_segment_size=1, max_segment_size=SIZE_MAX, seeds=None,
                                    device=0):
    """cilhip_connected_components_lists: the reference's "given neighbours" overloads (:20-160) over CSR lists -- of cilhip_radius_search3f
    (symmetric) or cilhip_knn3f (directed: weak components; offsets = arange(n + 1) * k) -- with an optional byte mask per entry"""
    L = capi.load()
    on_device = hasattr(idx, "is_cuda") and idx.is_cuda
    if on_device:
        import torch

        dev = idx.device
        if dev.index is not None:
            device = dev.index
        off = offsets.to(device=dev, dtype=torch.int64).contiguous()
        ix = idx.to(torch.int32).contiguous() if idx.dtype != torch.int32 else idx.contiguous()
        kp = None if keep is None else keep.to(device=dev, dtype=torch.uint8).contiguous()
        torch.cuda.synchronize(dev)
        a_off, a_idx, a_keep, total, mem = off.data_ptr(), ix.data_ptr(), None if kp is None else kp.data_ptr(), ix.numel(), capi.MEM_DEVICE
    else:
        dev = None
        off = np.ascontiguousarray(offsets, np.uint64)
        ix = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        kp = None if keep is None else np.ascontiguousarray(keep, np.uint8).reshape(-1)
        a_off, a_idx, a_keep, total, mem = off.ctypes.data, ix.ctypes.data, None if kp is None else kp.ctypes.data, ix.size, capi.MEM_HOST
    if len(off) != n + 1 or (kp is not None and len(kp) != total):
        raise ValueError("offsets must have n + 1 entries and keep one byte per list entry")
    sp, ns, skeep = _cc_seeds(seeds)
    outs, addr = _cc_outputs(n, on_device, dev)
    nseg = C.c_size_t(0)
    rc = L.cilhip_connected_components_lists(int(device), n, a_off, a_idx, a_keep, total, int(bool(skip_first)), int(bool(symmetric)), mem, int(min_segment_size),
                                             min(int(max_segment_size), SIZE_MAX), sp, ns, addr[0], addr[1], addr[2], C.byref(nseg))
    if rc != capi.OK:
        raise capi.CilhipError(rc, "cilhip_connected_components_lists: " + L.cilhip_last_error(None).decode())
    if n == 0:
        outs[1][:1] = 0
    return _cc_result(outs, nseg.value, on_device)


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
        names = ("evaluator", "min_segment_size", "max_segment_size")
        for k, v in zip(names, args):
            kw[k] = v
        self._labels, self._offsets, self._members = connected_components(self._points, nh.radius, kw.get("evaluator"), kw.get("min_segment_size", 1),
                                                                          kw.get("max_segment_size", SIZE_MAX), seeds, self._device)
        return self

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


def mean_shift(points, kernel_radius, max_iter, cluster_tol, convergence_tol=float(np.finfo(np.float32).eps), evaluator=None, seeds=None, form=0, device=0):
    """cilhip_mean_shift3f -> dict(shifted[ns, 3], labels[ns], modes[k, 3], offsets[k + 1], members[ns], iterations, stats): cluster c is
    members[offsets[c]:offsets[c + 1]]; seeds=None: every point is a seed"""
    L = capi.load()
    ev = evaluator if evaluator is not None else UnityWeightEvaluator()
    p, n, mem, keep_p = _as_cloud(points)
    sp, ns, keep_s = None, n, None
    if seeds is not None:
        sp, ns, smem, keep_s = _as_cloud(seeds)
        if smem != mem:
            raise ValueError("points and seeds must live in the same memory space")
        if ns == 0:
            sp = (np.zeros((1, 3), np.float32) if mem == capi.MEM_HOST else keep_s.new_zeros((1, 3)))
            keep_s = sp
            sp = sp.ctypes.data if mem == capi.MEM_HOST else sp.data_ptr()      # (an empty list is still a list: a non-null pointer)
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol, prm.convergence_tol = kernel_radius, int(max_iter), cluster_tol, convergence_tol
    prm.kernel_kind, prm.kernel_sigma, prm.form = int(ev.kind), float(ev.sigma), int(form)
    on_device = mem == capi.MEM_DEVICE
    if on_device:
        import torch

        dev = keep_p.device
        if dev.index is not None:
            device = dev.index
        torch.cuda.synchronize(dev)      # the call runs on a stream of its own: the inputs must be complete
        shifted, modes = torch.empty((ns, 3), dtype=torch.float32, device=dev), torch.empty((ns, 3), dtype=torch.float32, device=dev)
        labels, offsets, members = (torch.empty(k, dtype=torch.int32, device=dev) for k in (ns, ns + 1, ns))
        addr = [t.data_ptr() for t in (shifted, labels, modes, offsets, members)]
    else:
        shifted, modes = np.empty((ns, 3), np.float32), np.empty((ns, 3), np.float32)
        labels, offsets, members = (np.empty(k, np.uint32) for k in (ns, ns + 1, ns))
        addr = [a.ctypes.data for a in (shifted, labels, modes, offsets, members)]
    nc, iters = C.c_size_t(0), C.c_size_t(0)
    rc = L.cilhip_mean_shift3f(int(device), p, n, sp, ns if seeds is not None else 0, mem, C.byref(prm), addr[0], addr[1], addr[2], addr[3], addr[4], C.byref(nc), C.byref(iters))
    if rc != capi.OK:
        raise capi.CilhipError(rc, "cilhip_mean_shift3f: " + L.cilhip_last_error(None).decode())
    if ns == 0:
        offsets[:1] = 0
    st = capi.MsStats()
    L.cilhip_ms_last_stats(C.byref(st))
    stats = {"form_used": st.form_used, "est_ball": st.est_ball, "shift_ms": st.shift_ms, "group_ms": st.group_ms, "passes": st.passes, "rounds": st.rounds} if ns else {}
    lab, off, mem_ = _cc_result([labels, offsets, members], nc.value, on_device)
    return {"shifted": shifted, "labels": lab, "modes": modes[: nc.value], "offsets": off, "members": mem_, "iterations": int(iters.value), "stats": stats}


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
        self._r = mean_shift(self._points, seeds=seeds, device=self._device, **kw)
        return self

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
