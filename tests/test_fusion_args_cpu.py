"""CPU: what the map-fusion entries (cilhip_fuse_frame3f, cilhip_fusion_remove_unstable3f) answer before they have a device -- one row per
refusal of c_api.h, in the style of tests/test_stateless_entries_cpu.py, whose helpers are used here.  A row asserts the return code, that no
output was written, and that cilhip_last_error(NULL) names the family."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cilantro_amd import capi
from test_stateless_entries_cpu import Arr, Obj, NO_TEXT, TOO_MANY, _has_gpu, _take, cloud, knn, outputs, run, sentinel

OK, INVALID, NO_DEVICE = capi.OK, capi.ERR_INVALID, capi.ERR_NO_DEVICE
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
W, H, N, NF = 8, 6, 32, 40
K_OK = np.array([[10, 0, 3.5], [0, 10, 2.5], [0, 0, 1]], np.float32)
POSE_OK = np.eye(4, dtype=np.float32)
F32 = np.float32


def _params(**change):
    p = capi.FusionParams()
    capi.load().cilhip_fusion_default_params(C.byref(p))
    for k, v in change.items():
        setattr(p, k, v)
    o = Obj(p)
    o.out = False
    return o


def _model(rows):
    return dict(xyz=Arr(sentinel(3 * rows, F32), out=True), nrm=Arr(sentinel(3 * rows, F32), out=True), rgb=Arr(sentinel(3 * rows, F32), out=True),
                conf=Arr(sentinel(rows, F32), out=True))


def fuse(name, n_model=N, capacity=N + NF, n_frame=NF, w=W, h=H, mem=HOST, device=0, null=(), K=K_OK, pose=POSE_OK, params=None):
    a = _model(N + NF)
    a.update(fxyz=Arr(cloud(NF) + F32(0.5)), fnrm=Arr(cloud(NF, 1)), frgb=Arr(cloud(NF, 2)), pose=Arr(np.ascontiguousarray(np.asarray(pose, F32).T), "host"),
             K=Arr(np.ascontiguousarray(np.asarray(K, F32).T), "host"), params=_params(**(params or {})), n_out=Obj(C.c_size_t(0xA5A5)),
             counts=Obj(capi.FusionCounts(0xA5, 0xA5, 0xA5, 0xA5, 0xA5)))
    a = _take(a, null)
    return [device, a["xyz"], a["nrm"], a["rgb"], a["conf"], n_model, capacity, a["fxyz"], a["fnrm"], a["frgb"], n_frame, mem, a["pose"], a["K"], w, h, a["params"], a["n_out"],
            a["counts"]]


def unstable(name, n_model=N, mem=HOST, device=0, null=(), thresh=3.0):
    a = _take(dict(_model(N), n_out=Obj(C.c_size_t(0xA5A5))), null)
    return [device, a["xyz"], a["nrm"], a["rgb"], a["conf"], n_model, mem, C.c_float(thresh), a["n_out"]]


ENTRIES = {"cilhip_fuse_frame3f": fuse, "cilhip_fusion_remove_unstable3f": unstable}
FAMILY = {"cilhip_fuse_frame3f": b"fuse_frame", "cilhip_fusion_remove_unstable3f": b"fusion_remove_unstable"}
K_NAN, POSE_INF = K_OK.copy(), POSE_OK.copy()
K_NAN[1, 2] = np.nan
POSE_INF[0, 3] = np.inf
FF, RU = "cilhip_fuse_frame3f", "cilhip_fusion_remove_unstable3f"

REFUSED = (
    # NULL n_out, params, K or cam_pose
    [(FF, dict(null=(what,))) for what in ("n_out", "params", "K", "pose")]
    # any NULL model array with capacity > 0; any NULL frame array with n_frame > 0
    + [(FF, dict(null=(what,))) for what in ("xyz", "nrm", "rgb", "conf", "fxyz", "fnrm", "frgb")]
    # n_model > capacity
    + [(FF, dict(n_model=N + 1, capacity=N)), (FF, dict(n_model=1, capacity=0))]
    # sizes
    + [(FF, dict(n_model=TOO_MANY - 1, capacity=TOO_MANY)), (FF, dict(n_frame=TOO_MANY - 1)), (FF, dict(w=1 << 16, h=1 << 16)), (FF, dict(w=TOO_MANY - 1, h=1))]
    # unknown mem
    + [(e, dict(mem=m)) for e in ENTRIES for m in (2, -1)]
    # non-finite K, pose or params; negative thresholds
    + [(FF, dict(K=K_NAN)), (FF, dict(pose=POSE_INF))]
    + [(FF, dict(params={field: bad})) for field in ("fusion_dist_thresh", "occlusion_dist_thresh", "radial_factor", "fuse_max_angle_deg", "append_min_angle_deg",
                                                     "free_space_max_angle_deg") for bad in (float("nan"), float("inf"))]
    + [(FF, dict(params={field: -1.0})) for field in ("fusion_dist_thresh", "occlusion_dist_thresh", "fuse_max_angle_deg", "append_min_angle_deg", "free_space_max_angle_deg")]
    # remove_unstable
    + [(RU, dict(null=(what,))) for what in ("n_out", "xyz", "nrm", "rgb", "conf")] + [(RU, dict(n_model=TOO_MANY - 1))]
)
REACH_THE_DEVICE = [(e, dict()) for e in ENTRIES] + [(e, dict(mem=DEVICE)) for e in ENTRIES] + [(FF, dict(n_model=0)), (FF, dict(w=2, h=2))]
NEED_NO_DEVICE = [(FF, wh) for wh in (dict(w=0), dict(h=0), dict(w=0, h=0), dict(n_frame=0), dict(n_frame=0, null=("fxyz", "fnrm", "frgb")),
                                      dict(n_frame=0, n_model=0, capacity=0, null=("xyz", "nrm", "rgb", "conf")), dict(w=0, mem=DEVICE))]


def _id(row):
    return row[0][len("cilhip_"):] + "-" + ",".join("%s=%s" % (k, k if k in ("K", "pose") else v) for k, v in row[1].items())


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
    model_before = outputs(args)[:4]
    assert run(hip_lib, entry, args) == NO_DEVICE
    assert outputs(args)[:4] == model_before
    assert FAMILY[entry] in hip_lib.cilhip_last_error(None) and b"device" in hip_lib.cilhip_last_error(None)


@pytest.mark.parametrize("row", NEED_NO_DEVICE, ids=_id)
def test_nothing_to_fuse_needs_no_device(hip_lib, row):
    entry, change = row
    run(hip_lib, "cilhip_knn3f", knn("cilhip_knn3f", k=0))      # (a refusal: the slot has text)
    assert hip_lib.cilhip_last_error(None) != NO_TEXT
    args = ENTRIES[entry](entry, **change)
    model_before = [a.bytes() for a in args[1:5] if a is not None]
    assert run(hip_lib, entry, args) == OK
    assert [a.bytes() for a in args[1:5] if a is not None] == model_before
    assert args[-2].o.value == change.get("n_model", N)      # *n_out = n_model
    c = args[-1].o
    assert (c.visited, c.fused, c.appended, c.removed, c.untouched) == (0, 0, 0, 0, 0)
    assert hip_lib.cilhip_last_error(None) == NO_TEXT      # a call that passes its argument rules clears the slot


def test_an_empty_model_has_nothing_unstable(hip_lib):
    args = unstable(RU, n_model=0, null=("xyz", "nrm", "rgb", "conf"))
    assert run(hip_lib, RU, args) == OK and args[-1].o.value == 0


def test_counts_may_be_null(hip_lib):
    args = fuse(FF, w=0, null=("counts",))
    assert run(hip_lib, FF, args) == OK and args[-2].o.value == N


def test_default_params(hip_lib):
    p = capi.FusionParams(*([7.0] * 6))
    hip_lib.cilhip_fusion_default_params(C.byref(p))
    want = (F32(0.01), F32(0.025), F32(-0.5) / F32(120 * 120), F32(75), F32(105), F32(45))      # fusion.cpp:98-100, :192, :211, :223
    got = (p.fusion_dist_thresh, p.occlusion_dist_thresh, p.radial_factor, p.fuse_max_angle_deg, p.append_min_angle_deg, p.free_space_max_angle_deg)
    assert all(F32(g) == w for g, w in zip(got, want))
    hip_lib.cilhip_fusion_default_params(None)      # (ignored)


def test_cpp_mirror_and_example_compile():
    """cilantro_hip/fusion.hpp, its test program and examples/fusion.cpp build against the library; without arguments neither needs a device"""
    from test_components_refs_cpu import build_cpp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_cpp(os.path.join(root, "tests", "cpp", "test_fusion.cpp"), "test_fusion")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    example = build_cpp(os.path.join(root, "examples", "fusion.cpp"), "example_fusion")
    r = subprocess.run([example], capture_output=True, text=True)
    assert r.returncode == 0 and "PLY" in r.stdout
