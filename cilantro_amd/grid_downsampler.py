"""Python mirrors of cilantro's voxel-grid downsamplers on top of the C ABI (cilhip_grid_downsample3f; the arithmetic is
stated in include/cilantro_hip/c_api.h and DESIGN.md).

    ds = PointsNormalsGridDownsampler3f(points, normals, 0.005)        # core/grid_downsampler.hpp:46-132
    p, n = ds.getDownsampledPointsNormals(min_points_in_bin=1)
    cloud = grid_downsample(points, 0.005, normals=normals)           # utilities/point_cloud.hpp:247-266 (gridDownsample)

numpy arrays and torch tensors both: host arrays in -> numpy arrays out; device tensors in -> device tensors out, nothing
crosses the bus.  `parallel` keeps the one meaning that is reproducible: True (the reference's default) = bins in lexicographic
cell order, False = bins in order of first appearance; the sums are the same either way.  There is no CPU path: without a
usable device every entry raises CilhipError.
"""
import ctypes as C

import numpy as np

from . import _abi, capi


def _run(points, normals, colors, bin_size, min_points_in_bin, parallel, want_counts, device):
    """-> (points, normals or None, colors or None, counts or None), every array cut to the number of bins"""
    L = capi.load()
    p, n, mem, keep_p = _abi.cloud(points)
    ptrs, keep = [None, None], [keep_p]
    for k, att in enumerate((normals, colors)):
        if att is None:
            continue
        ap, an, amem, akeep = _abi.cloud(att)
        if an != n:
            raise ValueError("points, normals and colors must have the same number of rows")
        if amem != mem:
            raise ValueError("points, normals and colors must live in the same memory space")
        ptrs[k] = ap
        keep.append(akeep)
    device, dev = _abi.enter(keep_p, device)
    outs = [_abi.empty((n, 3), np.float32, dev), None if normals is None else _abi.empty((n, 3), np.float32, dev),
            None if colors is None else _abi.empty((n, 3), np.float32, dev), _abi.empty(n, np.uint32, dev) if want_counts else None]
    rows = C.c_size_t(0)
    # capacity = n always suffices: one call, no counting call before it
    rc = L.cilhip_grid_downsample3f(device, p, ptrs[0], ptrs[1], n, mem, C.c_float(bin_size), int(min_points_in_bin), 1 if parallel else 0,
                                    *[_abi.ptr(o) for o in outs], n, C.byref(rows))
    _abi.check(rc, "cilhip_grid_downsample3f", L)
    return tuple(_abi.cut(o, rows.value, n) for o in outs)


def grid_downsample(points, bin_size, normals=None, colors=None, min_points_in_bin=1, parallel=True, device=0):
    """PointCloud3f::gridDownsample (utilities/point_cloud.hpp:247-266) -> a dict shaped like ply_io.read_ply's:
    {"points", "normals" (or None), "colors" (or None)}"""
    p, n, c, _ = _run(points, normals, colors, bin_size, min_points_in_bin, parallel, False, device)
    return {"points": p, "normals": n, "colors": c}


class _GridDownsampler:
    """the one implementation behind the four names: the device pass runs once, here (as the reference builds its bins in the
    constructor); every getter is served from it -- min_points_in_bin only leaves rows out (grid_downsampler.hpp:26-33)"""

    def __init__(self, points, normals, colors, bin_size, parallel, device):
        self._p, self._n, self._c, self._cnt = _run(points, normals, colors, bin_size, 1, parallel, True, device)

    def getNumberOfOccupiedBins(self):
        return int(self._cnt.shape[0])

    def getBinPointCounts(self):
        return self._cnt

    def _sel(self, rows, min_points_in_bin):
        if int(min_points_in_bin) <= 1:
            return rows
        return rows[self._cnt >= int(min_points_in_bin)]

    def getDownsampledPoints(self, min_points_in_bin=1):
        return self._sel(self._p, min_points_in_bin)


class _WithNormals:
    def getDownsampledNormals(self, min_points_in_bin=1):
        return self._sel(self._n, min_points_in_bin)

    def getDownsampledPointsNormals(self, min_points_in_bin=1):
        return self._sel(self._p, min_points_in_bin), self._sel(self._n, min_points_in_bin)


class _WithColors:
    def getDownsampledColors(self, min_points_in_bin=1):
        return self._sel(self._c, min_points_in_bin)

    def getDownsampledPointsColors(self, min_points_in_bin=1):
        return self._sel(self._p, min_points_in_bin), self._sel(self._c, min_points_in_bin)


class PointsGridDownsampler3f(_GridDownsampler):
    """core/grid_downsampler.hpp:8-44"""

    def __init__(self, points, bin_size, parallel=True, device=0):
        super().__init__(points, None, None, bin_size, parallel, device)


class PointsNormalsGridDownsampler3f(_GridDownsampler, _WithNormals):
    """core/grid_downsampler.hpp:46-132"""

    def __init__(self, points, normals, bin_size, parallel=True, device=0):
        super().__init__(points, normals, None, bin_size, parallel, device)


class PointsColorsGridDownsampler3f(_GridDownsampler, _WithColors):
    """core/grid_downsampler.hpp:134-220"""

    def __init__(self, points, colors, bin_size, parallel=True, device=0):
        super().__init__(points, None, colors, bin_size, parallel, device)


class PointsNormalsColorsGridDownsampler3f(_GridDownsampler, _WithNormals, _WithColors):
    """core/grid_downsampler.hpp:222-340"""

    def __init__(self, points, normals, colors, bin_size, parallel=True, device=0):
        super().__init__(points, normals, colors, bin_size, parallel, device)

    def getDownsampledPointsNormalsColors(self, min_points_in_bin=1):
        return self._sel(self._p, min_points_in_bin), self._sel(self._n, min_points_in_bin), self._sel(self._c, min_points_in_bin)
