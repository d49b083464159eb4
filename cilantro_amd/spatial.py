"""Python mirror of cilantro's spatial module (spatial/convex_polytope.hpp, flat_convex_hull_3d.hpp, space_region.hpp) for float in 2 and 3
dimensions, on top of cilhip_convex_hull_* and cilhip_polytope(s)_* (rules H1-H5 and Q1-Q2 of c_api.h).

    hull = ConvexHull3f(points, True, True)          # (points, compute_topology, simplicial_facets, merge_tol)
    hull.getVertices(); hull.getVertexPointIndices(); hull.getFacetVertexIndices(); hull.getFacetHyperplanes(); hull.getArea(); hull.getVolume()
    hull.containsPoint(p); hull.getInteriorPointsIndexMask(cloud); hull.getInteriorPointIndices(cloud, offset)
    region = SpaceRegion3f([hull, other]).unionWith(third); region.getInteriorPointIndices(cloud)

points: a numpy array (results are numpy) or a device-resident torch tensor (the three point queries return tensors on the same device).  The
hull itself is small and always numpy.  compute_topology = False keeps the facet and neighbour lists empty, as the reference does.

Not built: the halfspace constructor's vertex enumeration, intersectionWith, SpaceRegion.complement / relativeComplement / getVolume -- they
need the QP of convex_hull_utilities.hpp:12-193 and a dual hull.  ConvexPolytope.from_halfspaces gives a polytope for queries only.
"""
import copy
import ctypes as C

import numpy as np

from . import _abi, capi
from ._abi import ptr as _ptr
from .principal_component_analysis import PrincipalComponentAnalysis

NOT_BUILT = "not built: it needs the QP of convex_hull_utilities.hpp:12-193 and a dual hull"


def _query(L, kind, hs_cols, poly_offsets, points, dim, offset, device):
    """hs_cols: F x (dim + 1) f32 (one halfspace per row: the C layout); kind: 'dist' | 'mask' | 'idx'"""
    r = _abi.rows(points, dim, "points", cast=True)
    p, n, mem = r.ptr, r.n, r.mem
    device, dev = _abi.enter(r.keep, device)
    hs_cols = np.ascontiguousarray(hs_cols, np.float32)
    po = np.ascontiguousarray(poly_offsets, np.uint32)
    if kind == "dist":
        F = int(hs_cols.shape[0])
        out = _abi.empty((F, n), np.float32, dev)
        _abi.check(L.cilhip_polytope_signed_distances(device, hs_cols.ctypes.data, F, p, n, dim, mem, _ptr(out)), "cilhip_polytope_signed_distances", L)
        return out
    if kind == "mask":
        out = _abi.empty(n, np.uint8, dev)
        rc = L.cilhip_polytopes_interior_mask(device, hs_cols.ctypes.data, po.ctypes.data, len(po) - 1, p, n, dim, mem, C.c_float(offset), _ptr(out))
        _abi.check(rc, "cilhip_polytopes_interior_mask", L)
        return out.bool() if dev is not None else out.astype(bool)
    out = _abi.empty(max(n, 1), np.uint32, dev)
    count = C.c_size_t(0)
    rc = L.cilhip_polytopes_interior_indices(device, hs_cols.ctypes.data, po.ctypes.data, len(po) - 1, p, n, dim, mem, C.c_float(offset), _ptr(out), max(n, 1), C.byref(count))
    _abi.check(rc, "cilhip_polytopes_interior_indices", L)
    return out[:count.value]


def _split_tform(dim, a, b=None):
    if b is None:
        T = np.asarray(a, np.float32)
        if T.shape != (dim + 1, dim + 1):
            raise ValueError("a transform is a (dim + 1) x (dim + 1) matrix, or a rotation and a translation")
        return T[:dim, :dim].copy(), T[:dim, dim].copy()
    return np.asarray(a, np.float32).reshape(dim, dim), np.asarray(b, np.float32).reshape(dim)


class ConvexPolytope:
    """ConvexPolytope<float, dim>: the points constructor (:40-45).  `dim` comes from the subclass (ConvexPolytope2f / 3f) or the keyword."""
    DIM = None

    def __init__(self, points=None, compute_topology=False, simplicial_facets=False, merge_tol=0.0, dim=None, device=0):
        self._L = capi.load()
        self.dim_ = int(dim if dim is not None else (self.DIM if self.DIM is not None else np.asarray(points).shape[1]))
        self._device = int(device)
        self._queries_only = False
        self.is_bounded_ = True
        if points is None:      # the default constructor: the empty polytope (:14-25), no device needed
            p, mem, n = np.zeros((1, self.dim_), np.float32), capi.MEM_HOST, 0
        else:
            r = _abi.rows(points, self.dim_, "points", cast=True)
            p, mem, n = r.keep, r.mem, r.n
            self._device, _ = _abi.enter(p, device)
        h, info = C.c_void_p(), capi.HullInfo()
        rc = self._L.cilhip_convex_hull_create(self._device, _ptr(p), n, self.dim_, mem, int(bool(simplicial_facets)), float(merge_tol), C.byref(h), C.byref(info))
        _abi.check(rc, "cilhip_convex_hull_create", self._L)
        try:
            d, V, Fh = self.dim_, info.n_vertices, info.n_halfspaces
            self.vertex_point_indices_ = np.zeros(V, np.uint32)
            self.vertices_ = np.zeros((V, d), np.float32)
            self._hs = np.zeros((Fh, d + 1), np.float32)
            fo, fi, fn = np.zeros(info.n_facets + 1, np.uint32), np.zeros(info.n_facet_indices, np.uint32), np.zeros(info.n_facet_indices, np.uint32)
            vo, vf = np.zeros(V + 1, np.uint32), np.zeros(info.n_vertex_facets, np.uint32)
            self.survivors_per_round_ = np.zeros(info.rounds, np.uint64)
            rc = self._L.cilhip_convex_hull_get(h, _ptr(self.vertex_point_indices_), _ptr(self.vertices_), _ptr(self._hs), _ptr(fo), _ptr(fi), _ptr(fn), _ptr(vo), _ptr(vf),
                                                _ptr(self.survivors_per_round_))
            _abi.check(rc, "cilhip_convex_hull_get", self._L)
        finally:
            self._L.cilhip_convex_hull_destroy(h)
        self.is_empty_ = bool(info.is_empty)
        self.area_, self.volume_ = float(info.area), float(info.volume)
        self.interior_point_ = np.array(info.interior_point[:self.dim_], np.float32)
        self.info_ = {k: getattr(info, k) for k, _ in capi.HullInfo._fields_ if k != "interior_point"}
        if compute_topology:
            self.faces_ = [fi[fo[k]:fo[k + 1]].tolist() for k in range(info.n_facets)]
            self.face_neighbor_faces_ = [fn[fo[k]:fo[k + 1]].tolist() for k in range(info.n_facets)]
            self.vertex_neighbor_faces_ = [vf[vo[k]:vo[k + 1]].tolist() for k in range(V)]
        else:
            self.faces_, self.face_neighbor_faces_, self.vertex_neighbor_faces_ = [], [], []
            self.vertex_point_indices_ = np.zeros(0, np.uint32)

    @classmethod
    def from_halfspaces(cls, halfspaces, dim=None, device=0):
        """(dim + 1) x F halfspaces, nrm . x + off <= 0 inside: a polytope for the point queries and transform only (no vertex enumeration)"""
        hs = np.asarray(halfspaces, np.float32)
        self = cls.__new__(cls)
        self._L = capi.load()
        self.dim_ = int(dim if dim is not None else (cls.DIM if cls.DIM is not None else hs.shape[0] - 1))
        if hs.ndim != 2 or hs.shape[0] != self.dim_ + 1:
            raise ValueError("halfspaces are a (dim + 1) x F array")
        self._device, self._queries_only, self.is_bounded_, self.is_empty_ = int(device), True, False, False
        self._hs = np.ascontiguousarray(hs.T)
        self.vertices_ = np.zeros((0, self.dim_), np.float32)
        self.vertex_point_indices_ = np.zeros(0, np.uint32)
        self.interior_point_ = np.full(self.dim_, np.nan, np.float32)
        self.area_ = self.volume_ = float("nan")
        self.faces_, self.face_neighbor_faces_, self.vertex_neighbor_faces_, self.info_ = [], [], [], {}
        return self

    def _no_vertices(self):
        if self._queries_only:
            raise capi.CilhipError(capi.ERR_UNSUPPORTED, "a polytope given by halfspaces has no vertices here: the vertex enumeration is " + NOT_BUILT)

    def getSpaceDimension(self):
        return self.dim_

    def isEmpty(self):
        return self.is_empty_

    def isBounded(self):
        self._no_vertices()
        return self.is_bounded_

    def getArea(self):
        self._no_vertices()
        return self.area_

    def getVolume(self):
        self._no_vertices()
        return self.volume_

    def getVertices(self):
        self._no_vertices()
        return self.vertices_

    def getFacetHyperplanes(self):
        """(dim + 1) x F, the reference's matrix"""
        return self._hs.T

    def getInteriorPoint(self):
        self._no_vertices()
        return self.interior_point_

    def getFacetVertexIndices(self):
        return self.faces_

    def getVertexNeighborFacets(self):
        return self.vertex_neighbor_faces_

    def getFacetNeighborFacets(self):
        return self.face_neighbor_faces_

    def getVertexPointIndices(self):
        return self.vertex_point_indices_

    def intersectionWith(self, *args, **kwargs):
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "ConvexPolytope.intersectionWith is " + NOT_BUILT)

    def containsPoint(self, point, offset=0.0):
        """:109-115, on the host: f32, ((h0 x + h1 y) + h2 z) + h3 > -offset fails"""
        p = np.asarray(point, np.float32).reshape(self.dim_)
        lim = -np.float32(offset)
        for h in self._hs:
            v = np.float32(h[0] * p[0]) + np.float32(h[1] * p[1])
            if self.dim_ == 3:
                v = np.float32(v) + np.float32(h[2] * p[2])
            if np.float32(v) + h[self.dim_] > lim:
                return False
        return True

    def getPointSignedDistancesFromFacets(self, points):
        """:117-121 -> F x n"""
        return _query(self._L, "dist", self._hs, [0, len(self._hs)], points, self.dim_, 0.0, self._device)

    def getInteriorPointsIndexMask(self, points, offset=0.0):
        return _query(self._L, "mask", self._hs, [0, len(self._hs)], points, self.dim_, offset, self._device)

    def getInteriorPointIndices(self, points, offset=0.0):
        return _query(self._L, "idx", self._hs, [0, len(self._hs)], points, self.dim_, offset, self._device)

    def transform(self, a, b=None):
        """:155-191, host f32: vertices and the interior point by (R, t), the halfspaces by [[R, 0], [-t^T R, 1]]"""
        if self.is_empty_:
            return self
        R, t = _split_tform(self.dim_, a, b)
        d = self.dim_
        self.vertices_ = (self.vertices_ @ R.T + t).astype(np.float32)
        self.interior_point_ = (R @ self.interior_point_ + t).astype(np.float32)
        H = np.zeros((d + 1, d + 1), np.float32)
        H[:d, :d] = R
        H[d, :d] = -(t @ R)
        H[d, d] = 1.0
        self._hs = np.ascontiguousarray((H @ self._hs.T).T.astype(np.float32))
        return self

    def transformed(self, a, b=None):
        return copy.deepcopy(self).transform(a, b)

    def __deepcopy__(self, memo):
        c = self.__class__.__new__(self.__class__)
        for k, v in self.__dict__.items():
            c.__dict__[k] = v if k == "_L" else copy.deepcopy(v, memo)
        return c


class ConvexPolytope2f(ConvexPolytope):
    DIM = 2


class ConvexPolytope3f(ConvexPolytope):
    DIM = 3


ConvexHull2f, ConvexHull3f = ConvexPolytope2f, ConvexPolytope3f


class FlatConvexHull3f:
    """flat_convex_hull_3d.hpp: the 2-D hull of the points' projection on their two leading principal directions"""

    def __init__(self, points, compute_topology=True, simplicial_facets=True, merge_tol=0.0, device=0):
        self._pca = PrincipalComponentAnalysis(points, device=device)
        flat = self._pca.project(points, 2)
        self._hull = ConvexHull2f(flat, compute_topology, simplicial_facets, merge_tol, device=device)
        v2 = self._hull.getVertices()
        self.vertices_3d_ = self._pca.reconstruct(v2) if len(v2) else np.zeros((0, 3), np.float32)

    def getHull2D(self):
        return self._hull

    def getVertices2D(self):
        return self._hull.getVertices()

    def getVertices3D(self):
        return self.vertices_3d_

    def getVertexPointIndices(self):
        return self._hull.getVertexPointIndices()

    def getFacetVertexIndices(self):
        return self._hull.getFacetVertexIndices()

    def getArea(self):
        return self._hull.getArea()

    def getVolume(self):
        return self._hull.getVolume()

    def isEmpty(self):
        return self._hull.isEmpty()

    def transform(self, a, b=None):
        """the 3-D vertices by (R, t); the 2-D hull is in the plane's own frame and stays"""
        R, t = _split_tform(3, a, b)
        self.vertices_3d_ = (self.vertices_3d_ @ R.T + t).astype(np.float32)
        return self


class SpaceRegion:
    """SpaceRegion<float, dim>: a union of convex polytopes (space_region.hpp)"""
    DIM = None

    def __init__(self, polytopes=(), dim=None, device=0):
        if isinstance(polytopes, ConvexPolytope):
            polytopes = [polytopes]
        self.polytopes_ = list(polytopes)
        self.dim_ = int(dim if dim is not None else (self.DIM if self.DIM is not None else (self.polytopes_[0].getSpaceDimension() if self.polytopes_ else 2)))
        for p in self.polytopes_:
            if p.getSpaceDimension() != self.dim_:
                raise ValueError("every polytope of a region has the region's dimension")
        self._device = int(device)
        self._L = capi.load()

    def unionWith(self, other):
        return self.__class__(self.polytopes_ + other.polytopes_, dim=self.dim_, device=self._device)

    def intersectionWith(self, *args, **kwargs):
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "SpaceRegion.intersectionWith is " + NOT_BUILT)

    def complement(self, *args, **kwargs):
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "SpaceRegion.complement is " + NOT_BUILT)

    def relativeComplement(self, *args, **kwargs):
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "SpaceRegion.relativeComplement is " + NOT_BUILT)

    def getVolume(self, *args, **kwargs):
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "SpaceRegion.getVolume is " + NOT_BUILT)

    def getSpaceDimension(self):
        return self.dim_

    def isEmpty(self):
        return all(p.isEmpty() for p in self.polytopes_)

    def isBounded(self):
        return all(p.isBounded() for p in self.polytopes_)

    def getConvexPolytopes(self):
        return self.polytopes_

    def getInteriorPoint(self):
        for p in self.polytopes_:
            if not p.isEmpty():
                return p.getInteriorPoint()
        return np.full(self.dim_, np.nan, np.float32)

    def containsPoint(self, point, offset=0.0):
        return any(p.containsPoint(point, offset) for p in self.polytopes_)

    def _packed(self):
        hs = [p._hs for p in self.polytopes_]
        offs = np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.uint32)
        cols = np.concatenate(hs, axis=0) if hs else np.zeros((0, self.dim_ + 1), np.float32)
        return cols, offs

    def getInteriorPointsIndexMask(self, points, offset=0.0):
        cols, offs = self._packed()
        return _query(self._L, "mask", cols, offs, points, self.dim_, offset, self._device)

    def getInteriorPointIndices(self, points, offset=0.0):
        cols, offs = self._packed()
        return _query(self._L, "idx", cols, offs, points, self.dim_, offset, self._device)

    def transform(self, a, b=None):
        for p in self.polytopes_:
            p.transform(a, b)
        return self

    def transformed(self, a, b=None):
        return self.__class__([p.transformed(a, b) for p in self.polytopes_], dim=self.dim_, device=self._device)


class SpaceRegion2f(SpaceRegion):
    DIM = 2


class SpaceRegion3f(SpaceRegion):
    DIM = 3
