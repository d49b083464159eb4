"""Python mirror of cilantro's MultidimensionalScaling (utilities/multidimensional_scaling.hpp) on top of cilhip_mds_embedding: the classical
embedding of n points from their n x n distance matrix, matrix-free on the device (rules M1-M5 of c_api.h).

    mds = MultidimensionalScaling(distances_sq, 2)                      # MultidimensionalScaling<float, 2>
    mds = MultidimensionalScaling(distances, 3, estimate_dim=True, distances_are_squared=False)
    mds.getEmbeddedPoints(); mds.getComputedEigenValues(); mds.getEmbeddingDimension()

The distances: a numpy array (the result is numpy) or a device-resident torch tensor (the embedding is a tensor on the same device).
"""
import ctypes as C

import numpy as np

from . import _abi, capi
from ._abi import ptr as _ptr


def _matrix(distances, device):
    """-> (the array to hand over, n, mem, device)"""
    if _abi.on_device(distances):
        import torch

        d, mem = distances.to(torch.float32).contiguous(), capi.MEM_DEVICE
    else:
        d, mem = np.ascontiguousarray(distances.cpu() if hasattr(distances, "cpu") else distances, np.float32), capi.MEM_HOST
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("a distance matrix is square")
    return d, int(d.shape[0]), mem, _abi.enter(d, device)[0]


def mds_embedding(distances, max_dim=2, estimate_dim=False, distances_are_squared=True, device=0, max_outer=None, degree=None, guard=None, raise_unconverged=True):
    """cilhip_mds_embedding -> (embedded[n, dim] f32, eigenvalues[nev] f32, result dict).  Raises when the solver gave up (n_converged <
    num_eigenvalues after max_outer iterations) unless raise_unconverged is False."""
    L = capi.load()
    d, n, mem, device = _matrix(distances, device)
    prm = capi.MdsParams()
    L.cilhip_mds_default_params(C.byref(prm))
    prm.max_dim, prm.estimate_dim, prm.distances_are_squared = int(max_dim), int(bool(estimate_dim)), int(bool(distances_are_squared))
    for key, v in (("max_outer", max_outer), ("degree", degree), ("guard", guard)):
        if v is not None:
            setattr(prm, key, int(v))
    room = max(min(int(max_dim), 16), 2)
    emb = _abi.empty((n, room), np.float32, d.device if mem == capi.MEM_DEVICE else None)
    ev = np.zeros(room + 1, np.float32)
    res = capi.MdsResult()
    rc = L.cilhip_mds_embedding(device, _ptr(d), n, mem, C.byref(prm), _ptr(emb), ev.ctypes.data, C.byref(res))
    _abi.check(rc, "cilhip_mds_embedding", L)
    info = {k: getattr(res, k) for k, _ in capi.MdsResult._fields_}
    if raise_unconverged and res.n_converged < res.num_eigenvalues:
        raise capi.CilhipError(capi.ERR_UNSUPPORTED, "cilhip_mds_embedding: %d of %d eigenpairs converged in %d outer iterations (largest residual %.3g)"
                               % (res.n_converged, res.num_eigenvalues, res.outer_iterations, res.max_residual))
    dim = int(res.dim)
    flat = emb.reshape(-1)[: n * dim]      # (point-major n x dim at the start of the buffer)
    return flat.reshape(n, dim), ev[: res.num_eigenvalues].copy(), info


def mds_apply(distances, x, distances_are_squared=True, device=0):
    """cilhip_mds_apply: y = B x for an n x b f64 block (numpy, or torch tensors on the matrix's device) -> (y, device milliseconds of the product)"""
    L = capi.load()
    d, n, mem, device = _matrix(distances, device)
    if mem == capi.MEM_DEVICE:
        import torch

        xs = x.to(device=d.device, dtype=torch.float64).contiguous().reshape(n, -1)
        y = torch.empty_like(xs)
        _abi.enter(xs, device)
    else:
        xs = np.ascontiguousarray(x, np.float64).reshape(n, -1)
        y = np.empty_like(xs)
    ms = C.c_double(0.0)
    rc = L.cilhip_mds_apply(device, _ptr(d), n, mem, int(bool(distances_are_squared)), _ptr(xs), int(xs.shape[1]), _ptr(y), C.byref(ms))
    _abi.check(rc, "cilhip_mds_apply", L)
    return y, ms.value


def estimateEmbeddingDimensionEigengap(eigenvalues, max_dim):
    """utilities/multidimensional_scaling.hpp:10-31, in f32"""
    ev = np.asarray(eigenvalues, np.float32)
    min_val, max_val, max_diff, max_ind = np.float32(np.inf), np.float32(-np.inf), np.float32(-np.inf), 0
    for i in range(len(ev) - 1):
        diff = np.float32(ev[i] - ev[i + 1])
        if diff > max_diff:
            max_diff, max_ind = diff, i
        min_val, max_val = min(min_val, ev[i]), max(max_val, ev[i])
    min_val, max_val = min(min_val, ev[-1]), max(max_val, ev[-1])
    if np.float32(max_val - min_val) < np.finfo(np.float32).eps:
        return int(max_dim)
    return max_ind + 1


class MultidimensionalScaling:
    """MultidimensionalScaling<float, Dynamic> (:86-120); MultidimensionalScaling2f / 3f below fix the dimension as the reference's typedefs do"""

    def __init__(self, distances, max_dim=2, estimate_dim=False, distances_are_squared=True, device=0, **solver):
        self.embedded_points_, self.computed_eigenvalues_, self.solver_result_ = mds_embedding(distances, max_dim, estimate_dim, distances_are_squared, device, **solver)

    def getEmbeddedPoints(self):
        """n x dim, point-major (the reference's column-major dim x n)"""
        return self.embedded_points_

    def getComputedEigenValues(self):
        return self.computed_eigenvalues_

    def getEmbeddingDimension(self):
        return int(self.embedded_points_.shape[1])

    def getSolverResult(self):
        return self.solver_result_


MultidimensionalScalingXf = MultidimensionalScaling


class MultidimensionalScaling2f(MultidimensionalScaling):
    def __init__(self, distances, distances_are_squared=True, device=0, **solver):
        super().__init__(distances, 2, False, distances_are_squared, device, **solver)


class MultidimensionalScaling3f(MultidimensionalScaling):
    def __init__(self, distances, distances_are_squared=True, device=0, **solver):
        super().__init__(distances, 3, False, distances_are_squared, device, **solver)
