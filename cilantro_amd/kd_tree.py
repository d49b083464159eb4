"""Python mirror of cilantro's dimension-generic KDTree (core/kd_tree.hpp:144-406: KDTree2f, KDTreeXf) on top of the C ABI
(cilhip_knn_nd, cilhip_radius_search_nd): exact, exhaustive search over n x dim float points, 1 <= dim <= 16.

    tree = KDTreeXf(features)                                   # n x dim, numpy or a device tensor
    idx, d2, cnt = tree.kNNSearch(queries, k)                    # rows padded with -1 / +inf; queries None: the tree's own points
    idx, d2, cnt = tree.kNNInRadiusSearch(queries, k, radius)    # radius is a SQUARED distance, as everywhere
    off, idx, d2 = tree.radiusSearch(queries, radius)            # query i owns idx[off[i]:off[i + 1]]
    idx, d2 = tree.nearestNeighborSearch(queries)
    tree.search(queries, KNNNeighborhoodSpecification(10))       # core/nearest_neighbors.hpp

Return shapes are KDTree3f's (normal_estimation.py).  Lists ascend by (squared distance, index): among exactly equal distances the lowest
index is named -- KDTree3f keeps the 3-D grid path and the reference's traversal order instead.  There is no CPU path.
"""
import ctypes as C

import numpy as np

from . import _abi, capi

MAX_DIM = 16


class RadiusNeighborhoodSpecification:
    """core/nearest_neighbors.hpp: the radius is the SQUARED distance, as in the reference"""

    def __init__(self, radius_sq):
        self.radius = float(radius_sq)


class KNNNeighborhoodSpecification:
    """core/nearest_neighbors.hpp: the k nearest"""

    def __init__(self, k):
        self.maxNumberOfNeighbors = int(k)


class KNNInRadiusNeighborhoodSpecification:
    """core/nearest_neighbors.hpp: the k nearest within a SQUARED radius"""

    def __init__(self, k, radius_sq):
        self.maxNumberOfNeighbors = int(k)
        self.radius = float(radius_sq)


class KDTree:
    """points: n x dim; dim None: the points' own width.  Nothing is built: every search is one exhaustive pass on the device."""

    def __init__(self, points, dim=None, device=0):
        self._L = capi.load()
        shape = tuple(points.shape) if hasattr(points, "shape") else np.shape(points)
        if len(shape) != 2:
            raise ValueError("points are an n x dim array")
        self._dim = int(shape[1]) if dim is None else int(dim)
        if shape[1] != self._dim:
            raise ValueError(f"points must have shape (N, {self._dim})")
        self._points = points
        self._device = device

    @property
    def dim(self):
        return self._dim

    def _rows(self, x):
        r = _abi.rows(x, self._dim)
        _abi.enter(r.keep, self._device)      # (for the synchronise alone: the call runs on self._device, as it always has)
        return r

    def _both(self, queries):
        r = self._rows(self._points)
        if queries is None:
            return r.ptr, r.n, None, r.n, r.mem, (r.keep,)
        q = self._rows(queries)
        if q.mem != r.mem:
            raise ValueError("reference points and queries must live in the same memory space")
        return r.ptr, r.n, q.ptr, q.n, r.mem, (r.keep, q.keep)

    def _search(self, queries, k, radius_sq):
        p, n, qp, nq, mem, keep = self._both(queries)
        k = int(k)
        idx = np.zeros((nq, max(k, 0)), np.uint32); d2 = np.zeros((nq, max(k, 0)), np.float32); cnt = np.zeros(nq, np.uint32)
        rc = self._L.cilhip_knn_nd(self._device, p, n, qp, nq, self._dim, mem, k, C.c_float(radius_sq), idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data)
        _abi.check(rc, "cilhip_knn_nd", self._L)
        out = idx.astype(np.int64)
        out[idx == capi.NONE_IDX] = -1
        return out, d2, cnt.astype(np.int64)

    def kNNSearch(self, queries, k):
        """queries None: the tree's own points"""
        return self._search(queries, k, np.inf)

    def kNNInRadiusSearch(self, queries, k, radius):
        return self._search(queries, k, float(radius))

    def nearestNeighborSearch(self, queries):
        idx, d2, _ = self._search(queries, 1, np.inf)
        return idx[:, 0], d2[:, 0]

    def radiusSearch(self, queries, radius):
        """every neighbour with squared distance < radius, ascending by (distance, index) -> (offsets int64 [nq + 1], indices int64 [total],
        squared distances f32 [total])"""
        p, n, qp, nq, mem, keep = self._both(queries)
        off = np.zeros(nq + 1, np.uint64)
        total = C.c_size_t(0)
        rc = self._L.cilhip_radius_search_nd(self._device, p, n, qp, nq, self._dim, mem, C.c_float(radius), off.ctypes.data, None, None, 0, C.byref(total))
        _abi.check(rc, "cilhip_radius_search_nd", self._L)
        idx = np.zeros(max(total.value, 1), np.uint32); d2 = np.zeros(max(total.value, 1), np.float32)
        if total.value:
            rc = self._L.cilhip_radius_search_nd(self._device, p, n, qp, nq, self._dim, mem, C.c_float(radius), off.ctypes.data, idx.ctypes.data, d2.ctypes.data,
                                                 total.value, C.byref(total))
            _abi.check(rc, "cilhip_radius_search_nd", self._L)
        return off.astype(np.int64), idx[: total.value].astype(np.int64), d2[: total.value]

    def search(self, queries, nh):
        """the reference's generic search(): dispatch on the neighbourhood specification"""
        if isinstance(nh, KNNInRadiusNeighborhoodSpecification):
            return self.kNNInRadiusSearch(queries, nh.maxNumberOfNeighbors, nh.radius)
        if isinstance(nh, KNNNeighborhoodSpecification):
            return self.kNNSearch(queries, nh.maxNumberOfNeighbors)
        if isinstance(nh, RadiusNeighborhoodSpecification):
            return self.radiusSearch(queries, nh.radius)
        raise TypeError("search() takes a KNN, KNNInRadius or Radius neighbourhood specification")


class KDTree2f(KDTree):
    def __init__(self, points, device=0):
        super().__init__(points, 2, device)


class KDTreeXf(KDTree):
    def __init__(self, points, device=0):
        super().__init__(points, None, device)
