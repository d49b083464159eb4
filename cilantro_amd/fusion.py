"""Map fusion of registered depth frames: the "Map" step of cilantro's examples/fusion.cpp (:147-236) and its cleanup_callback
(:51-59) on top of the C ABI (cilhip_fuse_frame3f, cilhip_fusion_remove_unstable3f; the rules are stated in
include/cilantro_hip/c_api.h and DESIGN.md section 16).

    surfels = SurfelMap3f()
    for rgb, depth in frames:
        points, normals, colors = RGBDImagesToPointsNormalsColors(rgb, depth, conv, K)      # image_conversions.py, CUDA tensors
        ...                                                                                  # localise: icp.py, projective ICP
        counts = surfels.fuse((points, normals, colors), cam_pose, K, 640, 480)
    surfels.removeUnstable(3.0)

The model's four arrays stay torch CUDA tensors between calls, grown by doubling; a call moves only the row count and the five
populations to the host.  There is no CPU path: without a usable device every entry raises CilhipError.
"""
import ctypes as C

import numpy as np

from . import _abi, capi
from ._abi import check as _ck, cloud as _as_cloud

COUNT_NAMES = ("visited", "fused", "appended", "removed", "untouched")


def default_params():
    """cilhip_fusion_default_params: the reference's thresholds (fusion.cpp:98-100, :192, :211, :223)"""
    p = capi.FusionParams()
    capi.load().cilhip_fusion_default_params(C.byref(p))
    return p


def _counts(c):
    return {name: int(getattr(c, name)) for name in COUNT_NAMES}


def fuse_frame(model, n_model, frame, cam_pose, K, w, h, params=None, device=0):
    """cilhip_fuse_frame3f on caller-owned arrays, in place -> (n_out, counts).  model: (xyz (cap, 3), normals (cap, 3), rgb (cap, 3), conf
    (cap,)), frame: (xyz, normals, rgb) -- all numpy float32 arrays (host memory) or all CUDA tensors (device memory).  A capacity that is too
    small raises CilhipError with nothing written."""
    L = capi.load()
    mp, cap, mem, keep_m = zip(*[_as_cloud(a) for a in model[:3]])
    fp, nf, fmem, keep_f = zip(*[_as_cloud(a) for a in frame])
    conf = model[3]
    if mem[0] == capi.MEM_DEVICE:
        if not (getattr(conf, "is_cuda", False) and conf.is_contiguous()):
            raise ValueError("the confidences must be a contiguous CUDA tensor like the model")
        conf_ptr, conf_rows = conf.data_ptr(), conf.shape[0]
        for a, k in zip(model[:3], keep_m):
            if k.data_ptr() != a.data_ptr():
                raise ValueError("the model tensors must be contiguous (edited in place)")
    else:
        if not (isinstance(conf, np.ndarray) and conf.dtype == np.float32 and conf.flags.c_contiguous):
            raise ValueError("the confidences must be a contiguous float32 array (edited in place)")
        conf_ptr, conf_rows = conf.ctypes.data, conf.shape[0]
        for a, k in zip(model[:3], keep_m):
            if k is not a:
                raise ValueError("the model arrays must be contiguous float32 arrays (edited in place)")
    if len(set(mem + fmem)) != 1 or len(set(cap + (conf_rows,))) != 1 or len(set(nf)) != 1:
        raise ValueError("the model's arrays must share one capacity, the frame's one size, and all must live in the same memory space")
    device, _ = _abi.enter(keep_m[0], device)
    p = params if params is not None else default_params()
    n_out, counts = C.c_size_t(0), capi.FusionCounts()
    pose, k = _abi.colmajor(cam_pose, 4), _abi.colmajor(K, 3)
    _ck(L.cilhip_fuse_frame3f(device, mp[0], mp[1], mp[2], conf_ptr, int(n_model), cap[0], fp[0], fp[1], fp[2], nf[0], mem[0], pose.ctypes.data, k.ctypes.data,
                              int(w), int(h), C.byref(p), C.byref(n_out), C.byref(counts)), "cilhip_fuse_frame3f")
    return n_out.value, _counts(counts)


class SurfelMap3f:
    """the model of examples/fusion.cpp: `model` (points, normals, colors) and `confidence`, resident on one device"""

    def __init__(self, device=0, params=None):
        self.device = int(device)
        self.params = params if params is not None else default_params()
        self._n = 0
        self._arrays = None      # [xyz, normals, rgb, conf] with `capacity` rows
        self._last = dict.fromkeys(COUNT_NAMES, 0)

    # ---- the model, as views of the resident tensors ----
    def size(self):
        return self._n

    def isEmpty(self):
        return self._n == 0

    def _view(self, i):
        import torch

        if self._arrays is None:
            return torch.empty((0, 3) if i < 3 else (0,), dtype=torch.float32, device=f"cuda:{self.device}")
        return self._arrays[i][: self._n]

    points = property(lambda self: self._view(0))
    normals = property(lambda self: self._view(1))
    colors = property(lambda self: self._view(2))
    confidence = property(lambda self: self._view(3))

    def capacity(self):
        return 0 if self._arrays is None else self._arrays[0].shape[0]

    def _reserve(self, rows):
        import torch

        if rows <= self.capacity():
            return
        rows = max(rows, 2 * self.capacity())
        new = [torch.empty((rows, 3) if i < 3 else (rows,), dtype=torch.float32, device=f"cuda:{self.device}") for i in range(4)]
        if self._arrays is not None:
            for a, b in zip(new, self._arrays):
                a[: self._n] = b[: self._n]
        self._arrays = new

    def fuse(self, frame, cam_pose, K, w, h):
        """fuse one frame (points, normals, colors in the camera frame: numpy arrays or CUDA tensors) seen from cam_pose -> counts"""
        import torch

        dev = torch.device(f"cuda:{self.device}")
        frame = tuple(a.to(dev) if hasattr(a, "is_cuda") else torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1, 3)).to(dev) for a in frame)
        self._reserve(self._n + min(frame[0].shape[0], int(w) * int(h)))
        if self._arrays is None:
            self._reserve(1)
        self._n, self._last = fuse_frame(self._arrays, self._n, frame, cam_pose, K, w, h, self.params, self.device)
        return dict(self._last)

    def removeUnstable(self, conf_thresh):
        """cleanup_callback (fusion.cpp:51-59): points whose confidence is below conf_thresh leave, in the order remove() leaves"""
        if self._n == 0:
            return self
        _abi.enter(self._arrays[0], self.device)
        n_out = C.c_size_t(0)
        a = self._arrays
        _ck(capi.load().cilhip_fusion_remove_unstable3f(self.device, a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), self._n, capi.MEM_DEVICE,
                                                        float(conf_thresh), C.byref(n_out)), "cilhip_fusion_remove_unstable3f")
        self._n = n_out.value
        return self

    def clear(self):
        self._n = 0
        return self

    def lastCounts(self):
        return dict(self._last)
