"""Python mirror of cilantro's PrincipalComponentAnalysis (core/principal_component_analysis.hpp with core/covariance.hpp) on top of
cilhip_pca_fit / cilhip_pca_project / cilhip_pca_reconstruct (rules P1-P5 of c_api.h).

    pca = PrincipalComponentAnalysis(points)                  # n x dim, 1 <= dim <= 16; or (points, subset=indices)
    pca.getDataMean(); pca.getDataCovariance(); pca.getEigenValues(); pca.getEigenVectors()
    low = pca.project(points, 2); back = pca.reconstruct(low)

points: a numpy array (results are numpy) or a device-resident torch tensor (project / reconstruct return tensors on the same device).  Mean,
covariance and eigenpairs are small and always numpy.  getEigenVectors() returns the reference's matrix: eigenvector c is COLUMN c.
"""
import ctypes as C

import numpy as np

from . import capi
from .clustering import _ptr


def _points(x, device, width=None):
    if hasattr(x, "is_cuda") and x.is_cuda:
        import torch

        if x.device.index is not None:
            device = x.device.index
        p = x.to(torch.float32).contiguous()
        torch.cuda.synchronize(x.device)
        mem = capi.MEM_DEVICE
    else:
        p = np.ascontiguousarray(x.cpu() if hasattr(x, "cpu") else x, np.float32)
        mem = capi.MEM_HOST
    if p.ndim != 2 or (width is not None and p.shape[1] != width):
        raise ValueError("points are an n x dim array")
    return p, mem, int(device)


class PrincipalComponentAnalysis:
    def __init__(self, data, subset=None, device=0):
        self._L = capi.load()
        p, mem, self._device = _points(data, device)
        n, D = int(p.shape[0]), int(p.shape[1])
        sub, n_sub = None, 0
        if subset is not None:
            if mem == capi.MEM_DEVICE:
                import torch

                sub = subset if hasattr(subset, "is_cuda") else torch.as_tensor(np.asarray(subset, np.int64))
                sub = sub.to(device=p.device, dtype=torch.int32).contiguous()      # (the low 32 bits: uint32 indices)
                torch.cuda.synchronize(p.device)
                n_sub = int(sub.numel())
            else:
                sub = np.ascontiguousarray(np.asarray(subset, np.int64) & 0xFFFFFFFF, np.uint32)
                n_sub = int(sub.size)
                if n_sub == 0:
                    sub = np.zeros(1, np.uint32)
        self.mean_, self.covariance_ = np.zeros(D, np.float32), np.zeros((D, D), np.float32)
        self.eigenvalues_, self._vectors = np.zeros(D, np.float32), np.zeros((D, D), np.float32)
        valid = C.c_int(0)
        rc = self._L.cilhip_pca_fit(self._device, _ptr(p), n, D, _ptr(sub), n_sub, mem, self.mean_.ctypes.data, self.covariance_.ctypes.data, self.eigenvalues_.ctypes.data,
                                    self._vectors.ctypes.data, C.byref(valid))
        if rc != capi.OK:
            raise capi.CilhipError(rc, "cilhip_pca_fit: " + self._L.cilhip_last_error(None).decode())
        self.valid_ = bool(valid.value)
        self._dim = D

    def isValid(self):
        """False: fewer than 2 samples -- everything is NaN (covariance.hpp:35-39)"""
        return self.valid_

    def getDataMean(self):
        return self.mean_

    def getDataCovariance(self):
        return self.covariance_

    def getEigenValues(self):
        return self.eigenvalues_

    def getEigenVectors(self):
        return self._vectors.T

    def _map(self, points, other, reconstruct):
        p, mem, device = _points(points, self._device, other if reconstruct else self._dim)
        m, out_w = int(p.shape[0]), (self._dim if reconstruct else int(other))
        if mem == capi.MEM_DEVICE:
            import torch

            out = torch.empty((m, out_w), dtype=torch.float32, device=p.device)
            torch.cuda.synchronize(p.device)
        else:
            out = np.empty((m, out_w), np.float32)
        if reconstruct:
            rc = self._L.cilhip_pca_reconstruct(device, _ptr(p), m, int(other), self._dim, mem, self.mean_.ctypes.data, self._vectors.ctypes.data, _ptr(out))
        else:
            rc = self._L.cilhip_pca_project(device, _ptr(p), m, self._dim, mem, self.mean_.ctypes.data, self._vectors.ctypes.data, int(other), _ptr(out))
        if rc != capi.OK:
            raise capi.CilhipError(rc, ("cilhip_pca_reconstruct: " if reconstruct else "cilhip_pca_project: ") + self._L.cilhip_last_error(None).decode())
        return out

    def project(self, points, target_dim):
        """:46-49 -> m x target_dim"""
        return self._map(points, int(target_dim), False)

    def reconstruct(self, points):
        """:59-62: m x source_dim -> m x dim"""
        return self._map(points, int(points.shape[1]), True)


PrincipalComponentAnalysis2f = PrincipalComponentAnalysis3f = PrincipalComponentAnalysisXf = PrincipalComponentAnalysis
