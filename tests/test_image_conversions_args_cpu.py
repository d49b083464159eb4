"""CPU: what the image-conversion entries (cilhip_depth_image_to_points3f, cilhip_points_to_depth_image3f, cilhip_points_to_index_map3f)
answer before they have a device -- one row per refusal of c_api.h, in the style of tests/test_stateless_entries_cpu.py, whose helpers
are used here.  A row asserts the return code, that no output was written, and that cilhip_last_error(NULL) names the family."""
import ctypes as C

import numpy as np
import pytest

from cilantro_amd import capi
from test_stateless_entries_cpu import Arr, Obj, NO_TEXT, TOO_MANY, _has_gpu, _take, cloud, knn, outputs, run, sentinel

OK, INVALID, NO_DEVICE = capi.OK, capi.ERR_INVALID, capi.ERR_NO_DEVICE
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
W, H, N = 8, 6, 64
K_OK = np.array([[10, 0, 3.5], [0, 10, 2.5], [0, 0, 1]], np.float32)


def _conv(raw_type=capi.DEPTH_U16, scale=1000.0, truncated=0, max_depth=3.0):
    return Obj(capi.DepthConverter(raw_type, scale, truncated, max_depth))


def _abi(K):
    return Arr(np.ascontiguousarray(np.asarray(K, np.float32).T), "host")


def to_points(name, w=W, h=H, mem=HOST, device=0, null=(), K=K_OK, conv=None, want_normals=1, capacity=None):
    conv = conv or {}
    a = _take(dict(depth=Arr(np.full(max(w * h, 1) if w * h < 1 << 20 else 1, 1500, np.uint16)), rgb=Arr(np.zeros(3 * max(W * H, 1), np.uint8)), conv=_conv(**conv), K=_abi(K),
                   xyz_out=Arr(sentinel(3 * W * H, np.float32), out=True), normals_out=Arr(sentinel(3 * W * H, np.float32), out=True),
                   rgb_out=Arr(sentinel(3 * W * H, np.float32), out=True), n_out=Obj(C.c_size_t(0xA5A5))), null)
    if a["conv"] is not None:
        a["conv"].out = False
    return [device, a["depth"], a["rgb"], w, h, mem, a["conv"], a["K"], None, 0, want_normals, a["xyz_out"], a["normals_out"], a["rgb_out"],
            W * H if capacity is None else capacity, a["n_out"]]


def to_depth(name, n=N, n_arg=None, w=W, h=H, mem=HOST, device=0, null=(), K=K_OK, conv=None):
    conv = conv or {}
    a = _take(dict(xyz=Arr(cloud(n) + np.float32(0.5)), rgb=Arr(cloud(n, 3)), conv=_conv(**conv), K=_abi(K), depth_out=Arr(sentinel(W * H, np.uint32), out=True),
                   rgb_out=Arr(sentinel(3 * W * H, np.uint8), out=True)), null)
    if a["conv"] is not None:
        a["conv"].out = False
    return [device, a["xyz"], a["rgb"], n if n_arg is None else n_arg, mem, None, a["K"], a["conv"], w, h, a["depth_out"], a["rgb_out"]]


def to_index(name, n=N, n_arg=None, w=W, h=H, mem=HOST, device=0, null=(), K=K_OK):
    a = _take(dict(xyz=Arr(cloud(n) + np.float32(0.5)), K=_abi(K), index_out=Arr(sentinel(W * H, np.uint32), out=True)), null)
    return [device, a["xyz"], n if n_arg is None else n_arg, mem, None, a["K"], w, h, a["index_out"]]


ENTRIES = {"cilhip_depth_image_to_points3f": to_points, "cilhip_points_to_depth_image3f": to_depth, "cilhip_points_to_index_map3f": to_index}
FAMILY = {"cilhip_depth_image_to_points3f": b"depth_image_to_points", "cilhip_points_to_depth_image3f": b"points_to_depth_image",
          "cilhip_points_to_index_map3f": b"points_to_index_map"}
WITH_CONV = ["cilhip_depth_image_to_points3f", "cilhip_points_to_depth_image3f"]
FROM_POINTS = ["cilhip_points_to_depth_image3f", "cilhip_points_to_index_map3f"]
K_NAN, K_SINGULAR = K_OK.copy(), K_OK.copy()
K_NAN[0, 2] = np.nan
K_SINGULAR[1] = K_SINGULAR[0]

REFUSED = (
    # NULL required arrays
    [("cilhip_depth_image_to_points3f", dict(null=(what,))) for what in ("depth", "n_out", "conv", "K", "xyz_out")]
    + [("cilhip_points_to_depth_image3f", dict(null=(what,))) for what in ("xyz", "conv", "K", "depth_out")]
    + [("cilhip_points_to_index_map3f", dict(null=(what,))) for what in ("xyz", "K", "index_out")]
    # want_normals or rgb without its output when capacity > 0
    + [("cilhip_depth_image_to_points3f", dict(null=("normals_out",))), ("cilhip_depth_image_to_points3f", dict(null=("rgb_out",))),
       ("cilhip_points_to_depth_image3f", dict(null=("rgb_out",)))]
    # unknown mem / raw_type
    + [(e, dict(mem=m)) for e in ENTRIES for m in (2, -1)]
    + [(e, dict(conv=dict(raw_type=r))) for e in WITH_CONV for r in (2, -1)]
    # the converter
    + [(e, dict(conv=dict(scale=s))) for e in WITH_CONV for s in (0.0, -1.0, float("inf"), float("nan"))]
    + [(e, dict(conv=dict(truncated=1, max_depth=float("nan")))) for e in WITH_CONV]
    # sizes
    + [(e, dict(w=1 << 16, h=1 << 16)) for e in ENTRIES]
    + [(e, dict(w=TOO_MANY - 1, h=1)) for e in ENTRIES]
    + [(e, dict(n_arg=TOO_MANY - 1)) for e in FROM_POINTS]
    # K
    + [(e, dict(K=K_NAN)) for e in ENTRIES]
    + [("cilhip_depth_image_to_points3f", dict(K=K_SINGULAR))]
)
REACH_THE_DEVICE = [(e, dict()) for e in ENTRIES] + [(e, dict(mem=DEVICE)) for e in ENTRIES] + [("cilhip_depth_image_to_points3f", dict(conv=dict(raw_type=capi.DEPTH_F32)))]
NEED_NO_DEVICE = [(e, wh) for e in ENTRIES for wh in (dict(w=0), dict(h=0), dict(w=0, h=0))]


def _id(row):
    return row[0][len("cilhip_"):] + "-" + ",".join("%s=%s" % (k, "K" if k == "K" else v) for k, v in row[1].items())


@pytest.mark.parametrize("row", REFUSED, ids=_id)
def test_argument_refusals(hip_lib, row):
    entry, change = row
    args = ENTRIES[entry](entry, **change)
    before = outputs(args)
    assert run(hip_lib, entry, args) == INVALID
    assert outputs(args) == before
    text = hip_lib.cilhip_last_error(None)
    assert text != NO_TEXT and FAMILY[entry] in text, text


@pytest.mark.parametrize("row", REACH_THE_DEVICE, ids=_id)
def test_without_a_device_every_entry_answers_no_device(hip_lib, row):
    if _has_gpu():
        pytest.skip("a GPU is present")
    entry, change = row
    args = ENTRIES[entry](entry, **change)
    before = outputs(args)
    assert run(hip_lib, entry, args) == NO_DEVICE
    assert outputs(args) == before
    assert FAMILY[entry] in hip_lib.cilhip_last_error(None) and b"device" in hip_lib.cilhip_last_error(None)


@pytest.mark.parametrize("row", NEED_NO_DEVICE, ids=_id)
def test_empty_images_need_no_device(hip_lib, row):
    entry, change = row
    run(hip_lib, "cilhip_knn3f", knn("cilhip_knn3f", k=0))      # (a refusal: the slot has text)
    assert hip_lib.cilhip_last_error(None) != NO_TEXT
    args = ENTRIES[entry](entry, **change)
    before = outputs(args)
    assert run(hip_lib, entry, args) == OK
    if entry == "cilhip_depth_image_to_points3f":
        assert args[-1].o.value == 0 and outputs(args)[:-1] == before[:-1]
    else:
        assert outputs(args) == before
    assert hip_lib.cilhip_last_error(None) == NO_TEXT      # a call that passes its argument rules clears the slot


@pytest.mark.parametrize("entry", FROM_POINTS)
def test_no_points_in_host_memory_give_the_empty_image_without_a_device(hip_lib, entry):
    args = ENTRIES[entry](entry, n=0, null=("xyz",))
    assert run(hip_lib, entry, args) == OK
    out = [a for a in args if isinstance(a, Arr) and a.out]
    if entry == "cilhip_points_to_index_map3f":
        assert (out[0].a[: W * H] == 0xFFFFFFFF).all()
    else:
        assert (out[0].a.view(np.uint16)[: W * H] == 0).all() and (out[0].a.view(np.uint16)[W * H:] == 0xA5A5).all()      # (u16: half of the sentinel buffer)
        assert (out[1].a == 0).all()


def test_set_projection_on_a_null_context(hip_lib):
    K = np.ascontiguousarray(K_OK.T)
    assert hip_lib.cilhip_set_projection(None, K.ctypes.data, 640, 480, None) == INVALID
    assert hip_lib.cilhip_set_projection(None, None, 0, 0, None) == INVALID


def test_default_converter(hip_lib):
    c = capi.DepthConverter(7, 0.0, 9, 0.0)
    hip_lib.cilhip_depth_default_converter(C.byref(c))
    assert (c.raw_type, c.scale, c.truncated) == (capi.DEPTH_U16, 1.0, 0) and c.max_depth == np.finfo(np.float32).max
    hip_lib.cilhip_depth_default_converter(None)      # (ignored)
