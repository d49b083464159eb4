"""CPU: what the affine warp-field entries (cilhip_warp_field_estimate_affine3f, _resample_affine3f, cilhip_warp_field_icp_run_affine)
answer before they have a device -- the refusals that need no handle, in the style of tests/test_warp_args_cpu.py: the return code, no
output written, cilhip_last_error(NULL) naming the family.  They are the rigid siblings' refusals with the same codes; the rules that
need a handle or a context (the parameters, the context's state: a context exists only on a device) are rows of
tests/test_gpu_warp_field_affine.py."""
import ctypes as C
import os
import re

import numpy as np

from cilantro_amd import capi
from test_stateless_entries_cpu import NO_TEXT

INVALID, HOST = capi.ERR_INVALID, capi.MEM_HOST
F32, N = np.float32, 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["cilhip_warp_field_estimate_affine3f", "cilhip_warp_field_resample_affine3f", "cilhip_warp_field_icp_run_affine"]


def params(L):
    p = capi.WarpParams()
    L.cilhip_warp_default_params(C.byref(p))
    return p


def test_symbols_present_and_declared():
    raw = C.CDLL(capi.LIB_PATH)
    assert all(n in capi.SYMBOLS and hasattr(raw, n) for n in NAMES)
    header = open(os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")).read()
    for n, sibling in zip(NAMES, ["cilhip_warp_field_estimate3f", "cilhip_warp_field_resample3f", "cilhip_warp_field_icp_run"]):
        # the same parameter list as the rigid sibling, token for token
        def signature(name):
            m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
            assert m, name
            return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1))).strip()

        assert signature(n) == signature(sibling)


def test_argtypes_match_the_rigid_siblings(hip_lib):
    assert hip_lib.cilhip_warp_field_estimate_affine3f.argtypes == hip_lib.cilhip_warp_field_estimate3f.argtypes
    assert hip_lib.cilhip_warp_field_resample_affine3f.argtypes == hip_lib.cilhip_warp_field_resample3f.argtypes
    assert hip_lib.cilhip_warp_field_icp_run_affine.argtypes == hip_lib.cilhip_warp_field_icp_run.argtypes


def test_estimate_refuses_a_null_handle(hip_lib):
    T, xyz, nn = np.full(16 * N, 7, F32), np.zeros((N, 3), F32), np.zeros(N, np.uint32)
    st = capi.WarpStats(7, 7, 7, 7.0, 7.0)
    p = params(hip_lib)
    rc = hip_lib.cilhip_warp_field_estimate_affine3f(None, xyz.ctypes.data, xyz.ctypes.data, N, xyz.ctypes.data, nn.ctypes.data, HOST, C.byref(p), T.ctypes.data, C.byref(st))
    text = hip_lib.cilhip_last_error(None)
    assert rc == INVALID and text != NO_TEXT and b"warp_field_estimate_affine" in text and (T == 7).all() and st.gn_iterations == 7


def test_resample_refuses_a_null_handle(hip_lib):
    T = np.full(16 * N, 7, F32)
    assert hip_lib.cilhip_warp_field_resample_affine3f(None, T.ctypes.data, T.ctypes.data, HOST) == INVALID
    assert b"warp_field_resample_affine" in hip_lib.cilhip_last_error(None) and (T == 7).all()


def test_loop_refuses_a_null_context(hip_lib):
    T, res, p = np.full(16 * N, 7, F32), capi.IcpResult(), params(hip_lib)
    assert hip_lib.cilhip_warp_field_icp_run_affine(None, None, C.byref(p), 3, 1e-3, 1.0, None, T.ctypes.data, None, C.byref(res)) == INVALID
    assert b"warp_field_icp_run_affine" in hip_lib.cilhip_last_error(None) and (T == 7).all()


def test_every_null_argument_of_the_loop_is_refused_before_the_field_is_read(hip_lib):
    """without a context the loop has nowhere to record an error but the thread's slot, and answers there"""
    p = params(hip_lib)
    for args in ((None, None, None), (None, None, C.byref(p))):
        assert hip_lib.cilhip_warp_field_icp_run_affine(*args, 3, 1e-3, 1.0, None, None, None, None) == INVALID
        assert b"warp_field_icp_run_affine" in hip_lib.cilhip_last_error(None)
        assert hip_lib.cilhip_warp_field_icp_run(*args, 3, 1e-3, 1.0, None, None, None, None) == INVALID
