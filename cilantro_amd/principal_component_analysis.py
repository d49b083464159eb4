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

from . import _abi, capi
from ._abi import ptr as _ptr


class PrincipalComponentAnalysis:
    def __init__(self, data, subset=None, device=0):
        self._L = capi.load()
        r = _abi.rows(data, what="points", cast=True)
        p, n, D, mem = r.keep, r.n, r.dim, r.mem
        self._device, _ = _abi.enter(p, device)
        sub, n_sub = None, 0
        if subset is not None:
            if mem == capi.MEM_DEVICE:
                import torch

                sub = subset if hasattr(subset, "is_cuda") else torch.as_tensor(np.asarray(subset, np.int64))
                sub = sub.to(device=p.device, dtype=torch.int32).contiguous()      # (the low 32 bits: uint32 indices)
                _abi.enter(sub, device)
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
        _abi.check(rc, "cilhip_pca_fit", self._L)
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
        r = _abi.rows(points, other if reconstruct else self._dim, "points", cast=True)
        p, m, mem = r.ptr, r.n, r.mem
        device, dev = _abi.enter(r.keep, self._device)
        out = _abi.empty((m, self._dim if reconstruct else int(other)), np.float32, dev)
        if reconstruct:
            rc = self._L.cilhip_pca_reconstruct(device, p, m, int(other), self._dim, mem, self.mean_.ctypes.data, self._vectors.ctypes.data, _ptr(out))
        else:
            rc = self._L.cilhip_pca_project(device, p, m, self._dim, mem, self.mean_.ctypes.data, self._vectors.ctypes.data, int(other), _ptr(out))
        _abi.check(rc, "cilhip_pca_reconstruct" if reconstruct else "cilhip_pca_project", self._L)
        return out

    def project(self, points, target_dim):
        """:46-49 -> m x target_dim"""
        return self._map(points, int(target_dim), False)

    def reconstruct(self, points):
        """:59-62: m x source_dim -> m x dim"""
        return self._map(points, int(points.shape[1]), True)


PrincipalComponentAnalysis2f = PrincipalComponentAnalysis3f = PrincipalComponentAnalysisXf = PrincipalComponentAnalysis
