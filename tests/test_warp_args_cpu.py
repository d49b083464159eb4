"""CPU: what the warp-field entries (cilhip_warp_field_create, _estimate3f, _resample3f, cilhip_transform_points_per_point3f,
cilhip_warp_field_icp_run) answer before they have a device -- one row per refusal of c_api.h, in the style of
tests/test_stateless_entries_cpu.py: the return code, no output written, cilhip_last_error(NULL) naming the family.  The rules that
need a handle (the parameters of estimate3f, the context's state in icp_run) are rows of tests/test_gpu_warp_field.py."""
import ctypes as C

import numpy as np
import pytest

from cilantro_amd import capi
from test_stateless_entries_cpu import NO_TEXT, _has_gpu

OK, INVALID, UNSUPPORTED, NO_DEVICE = capi.OK, capi.ERR_INVALID, capi.ERR_UNSUPPORTED, capi.ERR_NO_DEVICE
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
F32, NONE = np.float32, 0xFFFFFFFF
N, NC, KC, KR = 40, 6, 4, 3
SENTINEL = 0xA5A5A5A5


def lists():
    rng = np.random.default_rng(0)
    ci = rng.integers(0, NC, (N, KC)).astype(np.uint32)
    ri = np.stack([(np.arange(NC) + j) % NC for j in range(KR)], 1).astype(np.uint32)
    ci[3, 2:] = NONE
    return dict(ci=ci, cd=rng.random((N, KC), dtype=F32), ri=ri, rd=rng.random((NC, KR), dtype=F32))


def create(L, n_src=N, n_ctrl=NC, k_ctrl=KC, k_reg=KR, ctrl_kernel=1, ctrl_sigma=0.1, reg_kernel=1, reg_sigma=0.3, mem=HOST, device=0, null=(), bad_index=None, out=True):
    a = lists()
    if bad_index:
        a[bad_index[0]].reshape(-1)[bad_index[1]] = bad_index[2]
    p = {k: (None if k in null else v.ctypes.data) for k, v in a.items()}
    h = C.c_void_p(SENTINEL)
    rc = L.cilhip_warp_field_create(device, n_src, n_ctrl, p["ci"], p["cd"], k_ctrl, ctrl_kernel, ctrl_sigma, p["ri"], p["rd"], k_reg, reg_kernel, reg_sigma, mem,
                                    C.byref(h) if out else None)
    return rc, h.value


REFUSED = [
    dict(out=False), dict(null=("ci",)), dict(null=("cd",)), dict(null=("ri",)), dict(null=("rd",)),
    dict(n_ctrl=0), dict(n_src=0),
    dict(k_ctrl=0), dict(k_ctrl=33), dict(k_reg=0), dict(k_reg=33),
    dict(n_src=(1 << 32) // 4, k_ctrl=4),
    dict(ctrl_sigma=float("nan")), dict(ctrl_sigma=float("inf")), dict(reg_sigma=float("nan")), dict(reg_sigma=float("-inf")), dict(ctrl_sigma=0.0), dict(reg_sigma=0.0),
    dict(ctrl_kernel=0, ctrl_sigma=float("nan")),
    dict(mem=2), dict(mem=-1),
    dict(bad_index=("ci", 5, NC)), dict(bad_index=("ci", 7, 0xFFFFFFFE)), dict(bad_index=("ri", 4, NC + 3)),
]


@pytest.mark.parametrize("change", REFUSED, ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_create_refusals(hip_lib, change):
    rc, h = create(hip_lib, **change)
    assert rc == INVALID and h == SENTINEL
    text = hip_lib.cilhip_last_error(None)
    assert text != NO_TEXT and b"warp_field_create" in text, text


@pytest.mark.parametrize("change", [dict(ctrl_kernel=2), dict(reg_kernel=-1)], ids=str)
def test_unknown_kernel_codes_are_unsupported(hip_lib, change):
    rc, h = create(hip_lib, **change)
    assert rc == UNSUPPORTED and h == SENTINEL and b"warp_field_create" in hip_lib.cilhip_last_error(None)


@pytest.mark.parametrize("change", [dict(), dict(mem=DEVICE), dict(ctrl_kernel=0, reg_kernel=0, ctrl_sigma=0.0, reg_sigma=0.0)], ids=str)
def test_without_a_device_create_answers_no_device(hip_lib, change):
    if _has_gpu():
        pytest.skip("a GPU is present")
    rc, h = create(hip_lib, **change)
    assert rc == NO_DEVICE and h == SENTINEL
    assert b"warp_field_create" in hip_lib.cilhip_last_error(None) and b"device" in hip_lib.cilhip_last_error(None)


def test_entries_that_take_a_handle_refuse_null(hip_lib):
    T = np.full(16 * N, 7, F32)
    xyz = np.zeros((N, 3), F32)
    nn = np.zeros(N, np.uint32)
    p = capi.WarpParams()
    hip_lib.cilhip_warp_default_params(C.byref(p))
    st = capi.WarpStats(7, 7, 7, 7.0, 7.0)
    assert hip_lib.cilhip_warp_field_estimate3f(None, xyz.ctypes.data, xyz.ctypes.data, N, xyz.ctypes.data, nn.ctypes.data, HOST, C.byref(p), T.ctypes.data, C.byref(st)) == INVALID
    assert b"warp_field_estimate" in hip_lib.cilhip_last_error(None) and (T == 7).all() and st.gn_iterations == 7
    assert hip_lib.cilhip_warp_field_resample3f(None, T.ctypes.data, T.ctypes.data, HOST) == INVALID
    assert b"warp_field_resample" in hip_lib.cilhip_last_error(None) and (T == 7).all()
    res = capi.IcpResult()
    assert hip_lib.cilhip_warp_field_icp_run(None, None, C.byref(p), 3, 1e-3, 1.0, None, T.ctypes.data, None, C.byref(res)) == INVALID
    assert b"warp_field_icp_run" in hip_lib.cilhip_last_error(None) and (T == 7).all()
    hip_lib.cilhip_warp_field_destroy(None)      # (ignored)


def per_point(L, n=N, mem=HOST, device=0, null=()):
    a = dict(T=np.tile(np.eye(4, dtype=F32).reshape(-1), n if n < 1000 else 1), xyz=np.ones((min(n, 1000), 3), F32), out=np.full((min(n, 1000), 3), 7, F32))
    p = {k: (None if k in null else v.ctypes.data) for k, v in a.items()}
    return L.cilhip_transform_points_per_point3f(device, p["T"], p["xyz"], n, mem, p["out"]), a["out"]


@pytest.mark.parametrize("change", [dict(null=("T",)), dict(null=("xyz",)), dict(null=("out",)), dict(mem=3), dict(n=1 << 28)], ids=str)
def test_transform_points_refusals(hip_lib, change):
    rc, out = per_point(hip_lib, **change)
    assert rc == INVALID and (out == 7).all()
    assert b"transform_points_per_point" in hip_lib.cilhip_last_error(None)


def test_transform_points_of_nothing_needs_no_device(hip_lib):
    create(hip_lib, n_ctrl=0)      # (a refusal: the slot has text)
    assert hip_lib.cilhip_last_error(None) != NO_TEXT
    rc, _ = per_point(hip_lib, n=0, null=("T", "xyz", "out"))
    assert rc == OK and hip_lib.cilhip_last_error(None) == NO_TEXT
    if not _has_gpu():
        rc, out = per_point(hip_lib)
        assert rc == NO_DEVICE and (out == 7).all() and b"transform_points_per_point" in hip_lib.cilhip_last_error(None)


def test_default_params(hip_lib):
    p = capi.WarpParams(7.0, 7.0, 7.0, 7.0, 7, 7.0, 7, 7.0)
    hip_lib.cilhip_warp_default_params(C.byref(p))
    # icp_warp_field_combined_metric_sparse.hpp:67-74 (the class) and warp_field_estimation.hpp:1411-1415 (the estimator)
    assert (F32(p.w_p2p), F32(p.w_p2pl), F32(p.w_reg), F32(p.huber_boundary)) == (F32(0.0), F32(1.0), F32(1.0), F32(1e-4))
    assert (p.max_gn_iter, F32(p.gn_conv_tol), p.max_cg_iter, F32(p.cg_conv_tol)) == (10, F32(1e-5), 1000, F32(1e-5))
    hip_lib.cilhip_warp_default_params(None)      # (ignored)


def test_symbols_present():
    names = ["cilhip_warp_default_params", "cilhip_warp_field_create", "cilhip_warp_field_destroy", "cilhip_warp_field_estimate3f", "cilhip_warp_field_resample3f",
             "cilhip_transform_points_per_point3f", "cilhip_warp_field_icp_run"]
    raw = C.CDLL(capi.LIB_PATH)
    assert all(n in capi.SYMBOLS and hasattr(raw, n) for n in names)
