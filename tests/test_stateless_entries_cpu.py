"""CPU: what every stateless entry point (the calls of c_api.h that take `int device` instead of a context) answers before it has a
device -- one table, one row per entry and argument refusal, plus one valid call per entry.  The expected codes are what the entries
returned before csrc/stateless.hpp gave them one common opening; tests/test_gpu_stateless_entries.py imports the builders and the
out-of-range codes from here.

A row asserts the return code, that no output was written, and that cilhip_last_error(NULL) has text for the failure."""
import ctypes as C

import numpy as np
import pytest

from cilantro_amd import capi

OK, INVALID, UNSUPPORTED, NO_DEVICE = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED, capi.ERR_NO_DEVICE
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
N = 64                   # points of a row's cloud
TOO_MANY = 0xFFFFFFF1    # above the limit of the families that index with 32 bits less a margin (0xFFFFFFF0)
NO_TEXT = b"null context"


def _has_gpu():
    import torch

    return torch.cuda.is_available()


# ---- arguments -------------------------------------------------------------------------------------------------------
class Arr:
    """an array argument.  where = "mem": it lives where the call's `mem` says; "host": always a host array.  out: the call writes it"""

    def __init__(self, a, where="mem", out=False):
        self.a, self.where, self.out = np.ascontiguousarray(a), where, out

    def bytes(self):
        return self.a.tobytes()


class Obj:
    """a ctypes object passed by reference (a result struct, a size_t, a handle): on the host, written by the call"""

    out = True

    def __init__(self, o):
        self.o = o

    def bytes(self):
        return bytes(self.o)


def sentinel(count, dtype):
    a = np.empty(max(int(count), 1), dtype)
    a.view(np.uint8).fill(0xA5)
    return a


def cloud(n, seed=0):
    return np.random.default_rng(seed).random((max(n, 1), 3), dtype=np.float32)[:n]


def plane_cloud(n, seed=0):
    rng = np.random.default_rng(seed)
    P = rng.random((n, 3), dtype=np.float32)
    P[:, 2] = np.float32(0.2) * P[:, 0] + np.float32(0.3) * P[:, 1] + np.float32(0.004) * rng.standard_normal(n).astype(np.float32)
    P[::5, 2] += np.float32(0.5)      # every fifth point is off the plane
    return P


def pair_clouds(n, seed=0):
    from cilantro_amd import synthetic as syn

    rng = np.random.default_rng(seed)
    src = rng.random((n, 3), dtype=np.float32)
    dst = (src.astype(np.float64) @ syn.rot_xyz(0.1, -0.2, 0.3).T + np.array([0.05, -0.02, 0.1])).astype(np.float32)
    dst[::5] += np.float32(0.5)       # every fifth pair is an outlier
    return dst, src


def run(L, name, args, on_device=False):
    """L.<name>(*args) -> rc.  on_device: every "mem" array is copied to the device first and the written ones are copied back"""
    held, argv = [], []
    for a in args:
        if isinstance(a, Obj):
            argv.append(C.byref(a.o))
        elif isinstance(a, Arr):
            if on_device and a.where == "mem":
                import torch

                t = torch.from_numpy(a.a.view(np.uint8).reshape(-1).copy()).cuda()
                held.append((a, t))
                argv.append(t.data_ptr())
            else:
                argv.append(a.a.ctypes.data)
        else:
            argv.append(a)
    rc = getattr(L, name)(*argv)
    for a, t in held:
        if a.out:
            a.a.view(np.uint8).reshape(-1)[:] = t.cpu().numpy()
    return rc


def outputs(args):
    return [a.bytes() for a in args if isinstance(a, (Arr, Obj)) and a.out]


# ---- one builder per entry: keyword arguments name what a row changes ------------------------------------------------
def _take(a, null):
    for key in null:
        assert key in a, key
        a[key] = None
    return a


def kmeans(name, n=N, mem=HOST, device=0, k=4, n_arg=None, null=(), P=None):
    P = cloud(n) if P is None else P
    full = name in ("cilhip_kmeans3f", "cilhip_kmeans3f_ex")
    a = _take(dict(xyz=Arr(P), centroids=Arr(P[: max(k, 1)].copy(), "host", out=full), labels=Arr(sentinel(n, np.uint32), "host", out=True),
                   iters=Obj(C.c_size_t(0xA5A5))), null)
    n_ = n if n_arg is None else n_arg
    head = [device, a["xyz"], n_, mem, a["centroids"], k]
    return {"cilhip_kmeans3f": head + [5, 0.0, a["labels"], a["iters"]], "cilhip_kmeans3f_ex": head + [5, 0.0, 1, a["labels"], a["iters"]],
            "cilhip_kmeans3f_assign": head + [a["labels"]], "cilhip_kmeans3f_assign_ex": head + [1, a["labels"]]}[name]


def kmeans_shard(name, n=N, mem=HOST, device=0, k=4, n_arg=None, null=(), P=None):
    a = _take(dict(xyz=Arr(cloud(n) if P is None else P), handle=Obj(C.c_void_p(0xA5A5A5A5))), null)
    return [device, a["xyz"], n if n_arg is None else n_arg, mem, k, 0, a["handle"]]


def ransac(name, n=N, mem=HOST, device=0, n_arg=None, null=(), samples=None, seed=7, max_iter=8, P=None, target=None):
    if name == "cilhip_plane_ransac3f":
        clouds, model = [Arr(plane_cloud(n) if P is None else P)], capi.PlaneModel()
    else:
        clouds, model = [Arr(x) for x in (pair_clouds(n) if P is None else P)], capi.TransformModel()
    C.memset(C.byref(model), 0xA5, C.sizeof(model))
    a = _take(dict(xyz=clouds[0], out=Obj(model), residuals=Arr(sentinel(n, np.float32), "host", out=True), inliers=Arr(sentinel(n, np.uint32), "host", out=True)), null)
    s = None if samples is None else Arr(np.asarray(samples, np.uint32), "host")
    return [device, a["xyz"]] + clouds[1:] + [n if n_arg is None else n_arg, mem, s, seed, 0.02, n // 2 if target is None else target, max_iter, 1, a["out"], a["residuals"],
                                             a["inliers"]]


def score(name, n=N, mem=HOST, device=0, n_arg=None, null=(), m=3, P=None):
    if name == "cilhip_plane_score3f":
        clouds, models = [Arr(plane_cloud(n) if P is None else P)], np.tile(np.array([0.0, 0.0, 1.0, -0.3], np.float32), (max(m, 1), 1))
        models[:, 3] -= np.float32(0.1) * np.arange(max(m, 1), dtype=np.float32)
    else:
        clouds, models = [Arr(x) for x in (pair_clouds(n) if P is None else P)], np.tile(np.eye(4, dtype=np.float32).reshape(-1), (max(m, 1), 1))
        models[:, 12] = np.float32(0.05) * np.arange(max(m, 1), dtype=np.float32)
    a = _take(dict(xyz=clouds[0], models=Arr(models, "host"), counts=Arr(sentinel(m, np.uint32), "host", out=True)), null)
    return [device, a["xyz"]] + clouds[1:] + [n if n_arg is None else n_arg, mem, a["models"], m, 0.05, a["counts"]]


def fit(name, n=N, mem=HOST, device=0, n_arg=None, null=(), P=None):
    if name == "cilhip_plane_fit3f":
        clouds, width = [Arr(plane_cloud(n) if P is None else P)], 4
    else:
        clouds, width = [Arr(x) for x in (pair_clouds(n) if P is None else P)], 16
    a = _take(dict(xyz=clouds[0], out=Arr(sentinel(width, np.float32), "host", out=True)), null)
    return [device, a["xyz"]] + clouds[1:] + [n if n_arg is None else n_arg, mem, a["out"]]


def knn(name, n=N, mem=HOST, device=0, k=4, n_arg=None, nq_arg=None, null=(), nq=None, P=None):
    nq = max(n // 2, 1) if nq is None else nq
    a = _take(dict(ref=Arr(cloud(n) if P is None else P), query=Arr(cloud(nq, 1)), idx=Arr(sentinel(nq * k, np.uint32), "host", out=True),
                   d2=Arr(sentinel(nq * k, np.float32), "host", out=True), counts=Arr(sentinel(nq, np.uint32), "host", out=True)), null)
    return [device, a["ref"], n if n_arg is None else n_arg, a["query"], nq if nq_arg is None else nq_arg, mem, k, float("inf"), a["idx"], a["d2"], a["counts"]]


def radius_search(name, n=N, mem=HOST, device=0, n_arg=None, nq_arg=None, null=(), nq=None, radius_sq=0.05 ** 2, P=None):
    nq = max(n // 2, 1) if nq is None else nq
    cap = 64 * nq + 64
    a = _take(dict(ref=Arr(cloud(n) if P is None else P), query=Arr(cloud(nq, 1)), offsets=Arr(sentinel(nq + 1, np.uint64), "host", out=True),
                   idx=Arr(sentinel(cap, np.uint32), "host", out=True), d2=Arr(sentinel(cap, np.float32), "host", out=True), total=Obj(C.c_size_t(0xA5A5))), null)
    return [device, a["ref"], n if n_arg is None else n_arg, a["query"], nq if nq_arg is None else nq_arg, mem, radius_sq, a["offsets"], a["idx"], a["d2"], cap, a["total"]]


def normals(name, n=N, mem=HOST, device=0, k=5, n_arg=None, null=(), radius_sq=0.1 ** 2, max_sq_dist=float("inf"), P=None):
    a = _take(dict(xyz=Arr(cloud(n) if P is None else P), normals=Arr(sentinel(3 * n, np.float32), "host", out=True), curvature=Arr(sentinel(n, np.float32), "host", out=True)), null)
    if name == "cilhip_normals_knn3f":
        return [device, a["xyz"], n if n_arg is None else n_arg, mem, k, max_sq_dist, None, a["normals"], a["curvature"]]
    return [device, a["xyz"], n if n_arg is None else n_arg, mem, radius_sq, None, a["normals"], a["curvature"]]


def grid_downsample(name, n=N, mem=HOST, device=0, n_arg=None, null=(), bin_size=0.1, P=None):
    P = cloud(n) if P is None else P
    a = _take(dict(xyz=Arr(P), normals=Arr(cloud(n, 2)), rgb=Arr(cloud(n, 3)), xyz_out=Arr(sentinel(3 * n, np.float32), out=True), normals_out=Arr(sentinel(3 * n, np.float32), out=True),
                   rgb_out=Arr(sentinel(3 * n, np.float32), out=True), counts=Arr(sentinel(n, np.uint32), out=True), n_out=Obj(C.c_size_t(0xA5A5))), null)
    return [device, a["xyz"], a["normals"], a["rgb"], n if n_arg is None else n_arg, mem, bin_size, 1, 1, a["xyz_out"], a["normals_out"], a["rgb_out"], a["counts"], n, a["n_out"]]


def _cc_outputs(n):
    return dict(labels=Arr(sentinel(n, np.uint32), out=True), offsets_out=Arr(sentinel(n + 1, np.uint32), out=True), members=Arr(sentinel(n, np.uint32), out=True),
                n_segments=Obj(C.c_size_t(0xA5A5)))


def components(name, n=N, mem=HOST, device=0, n_arg=None, null=(), radius_sq=0.08 ** 2, seeds=None, P=None):
    p = capi.CcParams()
    capi.load().cilhip_cc_default_params(C.byref(p))
    p.radius_sq, p.use_normals, p.max_angle, p.use_colors, p.color_thresh = radius_sq, 1, 3.0, 1, 2.0
    nrm = cloud(n, 2) + np.float32(0.1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a = _take(dict(xyz=Arr(cloud(n) if P is None else P), normals=Arr(nrm.astype(np.float32)), rgb=Arr(cloud(n, 3)), params=Obj(p), **_cc_outputs(n)), null)
    if a["params"] is not None:
        a["params"].out = False      # (read only)
    s = None if seeds is None else Arr(np.asarray(seeds, np.uint32), "host")
    return [device, a["xyz"], a["normals"], a["rgb"], n if n_arg is None else n_arg, mem, a["params"], s, 0 if seeds is None else len(seeds), a["labels"], a["offsets_out"],
            a["members"], a["n_segments"]]


def components_lists(name, n=N, mem=HOST, device=0, n_arg=None, null=(), seeds=None, symmetric=0):
    k = 3
    idx = np.random.default_rng(4).integers(0, max(n, 1), size=n * k, dtype=np.uint32)
    a = _take(dict(offsets=Arr(np.arange(n + 1, dtype=np.uint64) * k), idx=Arr(idx), **_cc_outputs(n)), null)
    s = None if seeds is None else Arr(np.asarray(seeds, np.uint32), "host")
    return [device, n if n_arg is None else n_arg, a["offsets"], a["idx"], None, n * k, 0, symmetric, mem, 1, 0xFFFFFFFF, s, 0 if seeds is None else len(seeds), a["labels"],
            a["offsets_out"], a["members"], a["n_segments"]]


ENTRIES = {
    "cilhip_kmeans3f": kmeans, "cilhip_kmeans3f_assign": kmeans, "cilhip_kmeans3f_ex": kmeans, "cilhip_kmeans3f_assign_ex": kmeans, "cilhip_kmeans_shard_create": kmeans_shard,
    "cilhip_plane_ransac3f": ransac, "cilhip_plane_score3f": score, "cilhip_plane_fit3f": fit,
    "cilhip_transform_ransac3f": ransac, "cilhip_transform_score3f": score, "cilhip_transform_fit3f": fit,
    "cilhip_knn3f": knn, "cilhip_radius_search3f": radius_search, "cilhip_normals_knn3f": normals, "cilhip_normals_radius3f": normals,
    "cilhip_grid_downsample3f": grid_downsample, "cilhip_connected_components3f": components, "cilhip_connected_components_lists": components_lists,
}
# what an entry answers to a device index that is not one of the machine's devices (there ARE devices): the k-means family has its own
DEVICE_OUT_OF_RANGE = {name: (INVALID if "kmeans" in name else NO_DEVICE) for name in ENTRIES}
# the text of these two families names them
NAMES_ITSELF = {"cilhip_grid_downsample3f": b"grid_downsample", "cilhip_connected_components3f": b"connected_components", "cilhip_connected_components_lists": b"connected_components"}

BAD_SAMPLES = np.tile(np.array([0, 1, N], np.uint32), 8)      # index N in a cloud of N points
KMEANS = [n for n in ENTRIES if "kmeans3f" in n]
RANSAC = ["cilhip_plane_ransac3f", "cilhip_transform_ransac3f"]
WITH_MEM_RULE = list(NAMES_ITSELF)

# ---- the table -------------------------------------------------------------------------------------------------------
# rows refused by an argument rule: (entry, what the row changes, the code) -- the same answer with and without a device
REFUSED = (
    [(e, dict(null=("xyz",)), INVALID) for e in ENTRIES if e not in ("cilhip_knn3f", "cilhip_radius_search3f", "cilhip_connected_components_lists")]
    + [(e, dict(null=("ref",)), INVALID) for e in ("cilhip_knn3f", "cilhip_radius_search3f")]
    + [(e, dict(n_arg=TOO_MANY), INVALID) for e in ENTRIES if e not in WITH_MEM_RULE]
    + [(e, dict(nq_arg=TOO_MANY), INVALID) for e in ("cilhip_knn3f", "cilhip_radius_search3f")]
    + [(e, dict(n_arg=1 << 32), INVALID) for e in WITH_MEM_RULE]
    + [(e, dict(n_arg=0), INVALID) for e in KMEANS]
    # null outputs
    + [(e, dict(null=("centroids",)), INVALID) for e in KMEANS]
    + [("cilhip_kmeans_shard_create", dict(null=("handle",)), INVALID)]
    + [(e, dict(null=("out",)), INVALID) for e in RANSAC + ["cilhip_plane_fit3f", "cilhip_transform_fit3f"]]
    + [(e, dict(null=("counts",)), INVALID) for e in ("cilhip_plane_score3f", "cilhip_transform_score3f")]
    + [(e, dict(null=("models",)), INVALID) for e in ("cilhip_plane_score3f", "cilhip_transform_score3f")]
    + [("cilhip_knn3f", dict(null=("idx", "counts")), INVALID), ("cilhip_radius_search3f", dict(null=("offsets",)), INVALID)]
    + [(e, dict(null=("normals",)), INVALID) for e in ("cilhip_normals_knn3f", "cilhip_normals_radius3f")]
    + [("cilhip_grid_downsample3f", dict(null=("n_out",)), INVALID)]
    + [(e, dict(null=(what,)), INVALID) for e in ("cilhip_connected_components3f", "cilhip_connected_components_lists") for what in ("labels", "n_segments")]
    + [("cilhip_connected_components3f", dict(null=("params",)), INVALID), ("cilhip_connected_components3f", dict(null=("normals",)), INVALID),
       ("cilhip_connected_components3f", dict(null=("rgb",)), INVALID), ("cilhip_connected_components_lists", dict(null=("offsets",)), INVALID),
       ("cilhip_connected_components_lists", dict(null=("idx",)), INVALID)]
    # k
    + [("cilhip_knn3f", dict(k=0), INVALID), ("cilhip_knn3f", dict(k=33), INVALID), ("cilhip_normals_knn3f", dict(k=33), INVALID),
       ("cilhip_normals_knn3f", dict(k=0), INVALID)]      # (k = 0 is the radius form: refused for its infinite radius)
    + [(e, dict(k=0), INVALID) for e in KMEANS + ["cilhip_kmeans_shard_create"]]
    + [(e, dict(k=2049), UNSUPPORTED) for e in KMEANS + ["cilhip_kmeans_shard_create"]]
    # mem, where an entry has a rule for it
    + [(e, dict(mem=m), INVALID) for e in WITH_MEM_RULE for m in (2, -1)]
    # the families' own rules
    + [("cilhip_normals_radius3f", dict(radius_sq=float("inf")), INVALID), ("cilhip_radius_search3f", dict(radius_sq=float("nan")), INVALID),
       ("cilhip_grid_downsample3f", dict(bin_size=0.0), INVALID), ("cilhip_connected_components3f", dict(radius_sq=float("inf")), INVALID),
       ("cilhip_connected_components3f", dict(seeds=[N]), INVALID), ("cilhip_connected_components_lists", dict(seeds=[N], symmetric=1), INVALID),
       ("cilhip_connected_components_lists", dict(seeds=[0]), UNSUPPORTED)]
)
# rows that pass the argument rules and go to the device: without one, CILHIP_ERR_NO_DEVICE and nothing written
REACH_THE_DEVICE = (
    [(e, dict()) for e in ENTRIES]
    + [(e, dict(mem=DEVICE)) for e in ENTRIES]
    + [(e, dict(mem=m)) for e in ENTRIES if e not in WITH_MEM_RULE for m in (2, -1)]      # (these read any other value as "host")
    + [(e, dict(samples=BAD_SAMPLES)) for e in RANSAC]      # (the samples are looked at once the cloud is on the device)
    + [(e, dict(n=0, nq=1, null=("ref",))) for e in ("cilhip_knn3f", "cilhip_radius_search3f")]
    + [(e, dict(n=0, null=("xyz",))) for e in ("cilhip_plane_ransac3f", "cilhip_plane_fit3f", "cilhip_transform_ransac3f", "cilhip_transform_fit3f", "cilhip_normals_knn3f")]
)
# rows that are answered without a device
NEED_NO_DEVICE = [("cilhip_plane_score3f", dict(m=0)), ("cilhip_transform_score3f", dict(m=0)), ("cilhip_grid_downsample3f", dict(n=0)),
                  ("cilhip_connected_components3f", dict(n=0)), ("cilhip_connected_components_lists", dict(n=0))]


def _id(row):
    return row[0][len("cilhip_"):] + "-" + ",".join("%s=%s" % (k, "samples" if k == "samples" else v) for k, v in row[1].items())


def check_failure_text(L, entry):
    text = L.cilhip_last_error(None)
    assert text != NO_TEXT, entry
    assert NAMES_ITSELF.get(entry, b"") in text, (entry, text)


@pytest.mark.parametrize("row", REFUSED, ids=_id)
def test_argument_refusals(hip_lib, row):
    entry, change, code = row
    args = ENTRIES[entry](entry, **change)
    before = outputs(args)
    assert run(hip_lib, entry, args) == code
    if entry == "cilhip_kmeans_shard_create" and code == UNSUPPORTED:      # (the handle is reset before k is looked at: no shard either way)
        assert args[-1].o.value is None
    else:
        assert outputs(args) == before
    check_failure_text(hip_lib, entry)


@pytest.mark.parametrize("row", REACH_THE_DEVICE, ids=_id)
def test_without_a_device_every_entry_answers_no_device(hip_lib, row):
    if _has_gpu():
        pytest.skip("a GPU is present")
    entry, change = row
    args = ENTRIES[entry](entry, **change)
    before = outputs(args)
    assert run(hip_lib, entry, args) == NO_DEVICE
    if entry == "cilhip_kmeans_shard_create":
        assert args[-1].o.value is None
    elif entry == "cilhip_radius_search3f":      # (*total_out is reset with the argument rules; the arrays are untouched)
        assert outputs(args)[:-1] == before[:-1] and args[-1].o.value == 0
    else:
        assert outputs(args) == before
    check_failure_text(hip_lib, entry)
    assert b"device" in hip_lib.cilhip_last_error(None)


@pytest.mark.parametrize("row", NEED_NO_DEVICE, ids=_id)
def test_empty_calls_need_no_device(hip_lib, row):
    entry, change = row
    run(hip_lib, "cilhip_knn3f", knn("cilhip_knn3f", k=0))      # (a refusal: the slot has text)
    assert hip_lib.cilhip_last_error(None) != NO_TEXT
    args = ENTRIES[entry](entry, **change)
    assert run(hip_lib, entry, args) == OK
    if "score" not in entry:
        assert args[-1].o.value == 0      # zero rows / zero segments
    assert hip_lib.cilhip_last_error(None) == NO_TEXT      # a call that passes its argument rules clears the slot
