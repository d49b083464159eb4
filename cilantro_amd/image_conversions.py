"""Python mirrors of cilantro's core/image_point_cloud_conversions.hpp on top of the C ABI (cilhip_depth_image_to_points3f,
cilhip_points_to_depth_image3f, cilhip_points_to_index_map3f; the arithmetic is stated in include/cilantro_hip/c_api.h and DESIGN.md
section 14).

    conv = DepthValueConverter(1000.0)                                          # u16 millimetres (:7-24)
    points, normals = depthImageToPointsNormals(depth, conv, K)                 # :149-239
    depth, rgb = pointsColorsToRGBDImages(points, colors, K, conv, 640, 480)    # :774-815
    index = pointsToIndexMap(points, K, 640, 480)                               # :865-894, uint32, EMPTY where no point lands

K is a 3x3 matrix, extrinsics a 4x4 rigid transform (camera to world) or None.  Depth images are (h, w) arrays of uint16 or float32
(the dtype picks the converter's raw type), rgb images (h, w, 3) of uint8.  numpy arrays in -> numpy arrays out; CUDA tensors in ->
CUDA tensors out (a uint16 image may be handed over as an int16 tensor of the same bits).  There is no CPU path: without a usable device
every entry raises CilhipError.
"""
import ctypes as C

import numpy as np

from . import _abi, capi
from ._abi import check as _ck, ptr as _ptr

EMPTY = 0xFFFFFFFF


class DepthValueConverter:
    """DepthValueConverter<RawT, float> (:7-24): metric = (1 / scale) * raw"""

    truncated = False
    max_depth = float(np.finfo(np.float32).max)

    def __init__(self, scale=1.0):
        self.scale = float(scale)


class TruncatedDepthValueConverter(DepthValueConverter):
    """TruncatedDepthValueConverter<RawT, float> (:26-51): depths at or beyond max_depth read as 0"""

    truncated = True

    def __init__(self, scale=1.0, max_depth=float(np.finfo(np.float32).max)):
        super().__init__(scale)
        self.max_depth = float(max_depth)


def _conv(conv, raw_type):
    conv = DepthValueConverter() if conv is None else conv
    return capi.DepthConverter(raw_type, conv.scale, 1 if conv.truncated else 0, conv.max_depth)


def _image(img, what):
    """-> (pointer, shape, mem, keepalive, raw_type or None)"""
    if _abi.is_torch(img):
        import torch

        t = img.contiguous()
        names = {torch.float32: capi.DEPTH_F32, torch.int16: capi.DEPTH_U16, torch.uint8: None}
        if hasattr(torch, "uint16"):
            names[torch.uint16] = capi.DEPTH_U16
        if t.dtype not in names:
            raise TypeError(what + ": uint16 / int16 / float32 depth, uint8 rgb")
        if t.is_cuda:
            return _ptr(t), tuple(t.shape), capi.MEM_DEVICE, t, names[t.dtype]
        img = t.numpy()
    a = np.ascontiguousarray(img)
    if a.dtype == np.int16:      # (uint16 bits, as a CUDA int16 tensor carries them)
        a = a.view(np.uint16)
    if a.dtype == np.uint8:
        return _ptr(a), a.shape, capi.MEM_HOST, a, None
    if a.dtype not in (np.uint16, np.float32):
        raise TypeError(what + ": a depth image is uint16 or float32")
    return _ptr(a), a.shape, capi.MEM_HOST, a, capi.DEPTH_U16 if a.dtype == np.uint16 else capi.DEPTH_F32


def depth_image_to_points(depth, conv, K, extrinsics=None, rgb=None, keep_invalid=False, want_normals=False, device=0):
    """cilhip_depth_image_to_points3f -> (points, normals or None, colors or None), every array cut to the number of rows"""
    L = capi.load()
    dp, shape, mem, keep_d, raw_type = _image(depth, "depth")
    if raw_type is None or len(shape) != 2:
        raise ValueError("depth must be an (h, w) image of uint16 or float32")
    h, w = shape
    cp, keep_c = None, None
    if rgb is not None:
        cp, cshape, cmem, keep_c, craw = _image(rgb, "rgb")
        if craw is not None or tuple(cshape) != (h, w, 3):
            raise ValueError("rgb must be an (h, w, 3) image of uint8")
        if cmem != mem:
            raise ValueError("depth and rgb must live in the same memory space")
    n = w * h
    device, dev = _abi.enter(keep_d, device)
    outs = [_abi.empty((n, 3), np.float32, dev) if use else None for use in (True, want_normals, rgb is not None)]
    rows = C.c_size_t(0)
    c, k, e = _conv(conv, raw_type), _abi.colmajor(K, 3), _abi.colmajor(extrinsics, 4)
    _ck(L.cilhip_depth_image_to_points3f(device, dp, cp, w, h, mem, C.byref(c), _ptr(k), _ptr(e), 1 if keep_invalid else 0, 1 if want_normals else 0,
                                         *[_ptr(o) for o in outs], n, C.byref(rows)), "cilhip_depth_image_to_points3f", L)
    return tuple(_abi.cut(o, rows.value, n) for o in outs)


def points_to_depth_image(points, K, conv, w, h, extrinsics=None, colors=None, raw_type=np.uint16, device=0):
    """cilhip_points_to_depth_image3f -> (depth (h, w) of raw_type, rgb (h, w, 3) uint8 or None)"""
    L = capi.load()
    p, n, mem, keep_p = _abi.cloud(points)
    cp, keep_c = None, None
    if colors is not None:
        cp, cn, cmem, keep_c = _abi.cloud(colors)
        if cn != n or cmem != mem:
            raise ValueError("points and colors must have the same number of rows and live in the same memory space")
    raw = capi.DEPTH_U16 if np.dtype(raw_type) == np.uint16 else capi.DEPTH_F32
    if np.dtype(raw_type) not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise TypeError("raw_type: numpy.uint16 or numpy.float32")
    w, h = int(w), int(h)
    device, dev = _abi.enter(keep_p, device)
    depth = _abi.empty((h, w), raw_type, dev)
    rgb = None if colors is None else _abi.empty((h, w, 3), np.uint8, dev)
    c, k, e = _conv(conv, raw), _abi.colmajor(K, 3), _abi.colmajor(extrinsics, 4)
    _ck(L.cilhip_points_to_depth_image3f(device, p, cp, n, mem, _ptr(e), _ptr(k), C.byref(c), w, h, _ptr(depth), _ptr(rgb)), "cilhip_points_to_depth_image3f", L)
    return depth, rgb


def points_to_index_map(points, K, w, h, extrinsics=None, device=0):
    """cilhip_points_to_index_map3f -> (h, w) uint32 (a CUDA input gives an int32 tensor of the same bits), EMPTY where no point lands"""
    L = capi.load()
    p, n, mem, keep_p = _abi.cloud(points)
    w, h = int(w), int(h)
    device, dev = _abi.enter(keep_p, device)
    out = _abi.empty((h, w), np.uint32, dev)
    _ck(L.cilhip_points_to_index_map3f(device, p, n, mem, _ptr(_abi.colmajor(extrinsics, 4)), _ptr(_abi.colmajor(K, 3)), w, h, _ptr(out)), "cilhip_points_to_index_map3f", L)
    return out


# ---- the reference's names (conversions between images and clouds; the image size comes from the arrays) -------------
def depthImageToPoints(depth, conv, K, extrinsics=None, keep_invalid=False, device=0):
    """:53-147"""
    return depth_image_to_points(depth, conv, K, extrinsics, None, keep_invalid, False, device)[0]


def depthImageToPointsNormals(depth, conv, K, extrinsics=None, keep_invalid=False, device=0):
    """:149-349"""
    return depth_image_to_points(depth, conv, K, extrinsics, None, keep_invalid, True, device)[:2]


def RGBDImagesToPointsColors(rgb, depth, conv, K, extrinsics=None, keep_invalid=False, device=0):
    """:351-465"""
    p, _, c = depth_image_to_points(depth, conv, K, extrinsics, rgb, keep_invalid, False, device)
    return p, c


def RGBDImagesToPointsNormalsColors(rgb, depth, conv, K, extrinsics=None, keep_invalid=False, device=0):
    """:467-695"""
    return depth_image_to_points(depth, conv, K, extrinsics, rgb, keep_invalid, True, device)


def pointsToDepthImage(points, K, conv, w, h, extrinsics=None, raw_type=np.uint16, device=0):
    """:697-772"""
    return points_to_depth_image(points, K, conv, w, h, extrinsics, None, raw_type, device)[0]


def pointsColorsToRGBDImages(points, colors, K, conv, w, h, extrinsics=None, raw_type=np.uint16, device=0):
    """:774-863 -> (rgb, depth)"""
    d, c = points_to_depth_image(points, K, conv, w, h, extrinsics, colors, raw_type, device)
    return c, d


def pointsToIndexMap(points, K, w, h, extrinsics=None, device=0):
    """:865-934"""
    return points_to_index_map(points, K, w, h, extrinsics, device)
