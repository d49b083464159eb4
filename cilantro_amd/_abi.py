"""What every stateless wrapper does around its one cilhip_* call, written once: arrays and tensors in, outputs on the same side, the return
code out.  Private; imports capi, numpy and, lazily, torch.

    r = rows(points, 3, "clouds")                     # (ptr, n, dim, mem, keep) of an n x dim float32 array or tensor
    device, dev = enter(r.keep, device)               # the tensor's device index; waits for the work that produced it
    out = empty((r.n, 3), np.float32, dev)            # numpy for dev None, else a tensor on dev (uint words in int tensors)
    check(L.cilhip_xxx(device, r.ptr, r.n, r.mem, ptr(out)), "cilhip_xxx", L)
    return cut(out, m, r.n)                           # or widen(labels)

Two laws for a tensor that is not float32, as the wrappers have had them: cast=False raises TypeError (the 3-D clouds and KDTree), cast=True
converts (everything in D dimensions).  The texts of the errors follow the law.

enter() has no "do not synchronise" switch: the wrappers that never synchronised never took the tensor's device index either, so they simply
do not call it.  With a device tensor the library then runs on the `device` argument, not on the tensor's own index, and -- except where
noted -- without a synchronise, although it works on a stream of its own: a cloud that torch is still writing may be read half-written.
Kept as they were, for a later change to decide:
    normal_estimation.KDTree3f._search / .radiusSearch, NormalEstimation3f._run / ._run_radius, RobustNormalEstimation3f._run (device outputs)
    clustering.KMeans3f.cluster, clustering.kmeans_assign
    model_estimation.PlaneRANSACEstimator3f.estimate / .estimateModel / .countInliers
    distributed_models.HipKMeansShard (the shard's constructor)
    kd_tree.KDTree._both (synchronises, through enter(); keeps the `device` argument)
"""
from collections import namedtuple

import numpy as np

from . import capi

Rows = namedtuple("Rows", "ptr n dim mem keep")


def is_torch(x):
    return type(x).__module__.startswith("torch")


def on_device(x):
    return bool(getattr(x, "is_cuda", False))


def rows(x, width=None, what="points", cast=False, none_ok=False):
    """an n x dim float32 array, CPU tensor (host memory, no copy) or device tensor -> Rows; width: the dim to insist on"""
    if x is None and none_ok:
        return Rows(None, 0, 0, capi.MEM_HOST, None)
    if is_torch(x):
        import torch

        if not cast and x.dtype != torch.float32:
            raise TypeError(f"{what} must be float32")
        x = x.to(torch.float32).contiguous()
        a = x if x.is_cuda else x.numpy()
    else:
        a = np.ascontiguousarray(x, dtype=np.float32)
    if a.ndim != 2 or (width is not None and a.shape[1] != width):
        raise ValueError(f"{what} are an n x dim array" if cast else f"{what} must have shape (N, {width})")
    return Rows(ptr(a), int(a.shape[0]), int(a.shape[1]), capi.MEM_DEVICE if on_device(a) else capi.MEM_HOST, a)


def cloud(x):
    """the (N, 3) law of the ICP classes -> (pointer, n, mem, keepalive); None is an absent cloud"""
    r = rows(x, 3, "clouds", none_ok=True)
    return r.ptr, r.n, r.mem, r.keep


def enter(keep, device):
    """-> (device index, torch device or None): a device tensor names its own device, and torch's work on it is waited for"""
    if not on_device(keep):
        return int(device), None
    import torch

    dev = keep.device
    if dev.index is not None:
        device = dev.index
    torch.cuda.synchronize(dev)      # the call runs on a stream of its own: the inputs must be complete
    return int(device), dev


_WORDS = {"uint16": "int16", "uint32": "int32", "uint64": "int64"}      # (torch tensors carry unsigned words in the signed type)


def empty(shape, dtype, dev=None, zero=False):
    """an output buffer: a numpy array for dev None, else a torch tensor on dev"""
    dtype = np.dtype(dtype)
    if dev is None:
        return (np.zeros if zero else np.empty)(shape, dtype)
    import torch

    return (torch.zeros if zero else torch.empty)(shape, dtype=getattr(torch, _WORDS.get(dtype.name, dtype.name)), device=dev)


def ptr(a):
    return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)


def widen(a):
    """uint32 words -> int64, also out of an int32 tensor: without the sign"""
    if is_torch(a):
        import torch

        return a.to(torch.int64) & 0xFFFFFFFF
    return a.astype(np.int64)


def cut(o, m, n):
    """the first m of n rows; a copy when they are less than half (do not keep an input-sized buffer alive behind a small result)"""
    if o is None or 2 * m >= n:
        return None if o is None else o[:m]
    return o[:m].clone() if is_torch(o) else o[:m].copy()


def check(rc, name, L=None):
    """name: the entry, prefixed to the library's text (None: the text alone)"""
    if rc != capi.OK:
        raise capi.CilhipError(rc, (name + ": " if name else "") + (L or capi.load()).cilhip_last_error(None).decode())


def colmajor(M, k):
    """a k x k matrix in math layout (row, col) -> the k * k floats of Eigen's column-major one; None stays None"""
    return None if M is None else np.ascontiguousarray(np.asarray(M, dtype=np.float32).reshape(k, k).T).reshape(k * k)


def T_to_abi(T):
    return colmajor(np.asarray(T, dtype=np.float32), 4)


def T_from_abi(buf):
    return np.array(buf, dtype=np.float32).reshape(4, 4).T.copy()
