"""GPU: the host estimate entries over a stored correspondence set -- cilhip_estimate_point_to_point / _combined / _combined_two_sets /
_affine and the two host-driven loops built on them (cilhip_icp_run_two_sets, the affine cilhip_icp_run with affine_device_loop = 0) --
against tests/golden/estimate_entries.npz, BYTE FOR BYTE: dT, AtA, Atb, converged / ok, n_corr and the result structs.  The fixture was
recorded from this same module against the library as it was before the estimates shared one accumulation routine, one Gauss-Newton
loop and one un-centring (csrc/estimate.hip); these are the bit-pinned host paths of three reference classes, and host f64 arithmetic
in the same order gives the same bits: there is no tolerance.  An array that differs means the arithmetic was reordered.

Clouds: seeded (cilantro_amd/synthetic.py), target 4 097 points with normals, source 2 049 points (more than one block, no multiple of
one), sources of 1 and 0 points, a radius that leaves no correspondence.  Recording (a development switch): with
CILHIP_ESTIMATE_ENTRIES_RECORD=<path> the module writes what it computed to <path> instead of comparing."""
import ctypes as C
import os

import numpy as np
import pytest

from cilantro_amd import capi
from cilantro_amd import synthetic as syn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "estimate_entries.npz")
RECORD = os.environ.get("CILHIP_ESTIMATE_ENTRIES_RECORD")
I4 = np.eye(4, dtype=np.float32)
WEIGHTS = ((0.0, 1.0), (1.0, 0.0), (0.3, 0.7), (0.0, 0.0))


def _bytes(*parts):
    return np.frombuffer(b"".join(np.ascontiguousarray(p).tobytes() for p in parts), np.uint8)


def _p2p(ctx):
    T = np.zeros(16, np.float32); sums = np.zeros(16, np.float64); ok = C.c_int(-1)
    ctx._ck(ctx._L.cilhip_estimate_point_to_point(ctx._h, T.ctypes.data, sums.ctypes.data, C.byref(ok)))
    return _bytes(T, sums, np.int32(ok.value))


def _combined(ctx, w, max_iter, tol=1e-5):
    T = np.zeros(16, np.float32); AtA = np.zeros(36, np.float64); Atb = np.zeros(6, np.float64); cv = C.c_int(-1)
    ctx._ck(ctx._L.cilhip_estimate_combined(ctx._h, w[0], w[1], max_iter, tol, T.ctypes.data, AtA.ctypes.data, Atb.ctypes.data, C.byref(cv)))
    return _bytes(T, AtA, Atb, np.int32(cv.value))


def _two_sets(cp, cl, w, max_iter, tol=1e-5):
    T = np.zeros(16, np.float32); cv = C.c_int(-1)
    cp._ck(cp._L.cilhip_estimate_combined_two_sets(cp._h, cl._h, w[0], w[1], max_iter, tol, T.ctypes.data_as(C.c_void_p), C.byref(cv)))
    return _bytes(T, np.int32(cv.value))


def _affine(ctx, w, centered):
    T = np.zeros(16, np.float32); AtA = np.zeros(144, np.float64); Atb = np.zeros(12, np.float64); ok = C.c_int(-1); n = C.c_size_t(12345)
    ctx._ck(ctx._L.cilhip_estimate_affine(ctx._h, w[0], w[1], 1 if centered else 0, T.ctypes.data, AtA.ctypes.data, Atb.ctypes.data, C.byref(n), C.byref(ok)))
    return _bytes(T, AtA, Atb, np.uint64(n.value), np.int32(ok.value))


def _params(ctx, max_sq, iters, w=(0.3, 0.7), opt_iters=2):
    p = capi.IcpParams()
    ctx._L.cilhip_icp_default_params(C.byref(p))
    p.metric, p.w_p2p, p.w_p2pl, p.max_sq_dist, p.max_iter, p.conv_tol, p.max_opt_iter = capi.METRIC_COMBINED, w[0], w[1], float(max_sq), iters, 0.0, opt_iters
    return p


def _single_set(ctx, tag, out, weights=WEIGHTS, iters=(0, 1, 5)):
    if ctx.get_option("search_direction") == 0:      # (the Kabsch entry reads matches, not a pair list)
        out[tag + "/p2p"] = _p2p(ctx)
    for w in weights:
        for it in iters:
            out[f"{tag}/combined w={w[0]},{w[1]} it={it}"] = _combined(ctx, w, it)
    for w, centered in (((1.0, 0.0), False), ((1.0, 0.0), True), ((0.3, 0.7), True), ((0.3, 0.7), False), ((0.0, 0.0), True)):
        out[f"{tag}/affine w={w[0]},{w[1]} centered={int(centered)}"] = _affine(ctx, w, centered)


@pytest.fixture(scope="module")
def computed(hip_lib):
    from cilantro_amd.icp import Context

    d = syn.make_pair(4097, 2049)
    D, N, S, r2 = d["dst"], d["dst_n"], d["src"], float(d["max_sq_dist"])
    SN = syn.make_normals(len(S), seed=47)
    out = {}
    ctx = Context()
    ctx.set_target(D, N)
    ctx.set_source(S)
    out["found"] = _bytes(np.uint64(ctx.find_correspondences(I4, r2)))
    _single_set(ctx, "unity", out)
    # RBF evaluators: the metric weights travel inside the per-pair weights
    for k, v in (("point_weight_evaluator", 2), ("plane_weight_evaluator", 2), ("point_weight_sigma", 0.05), ("plane_weight_sigma", 0.08)):
        ctx.set_option(k, v)
    _single_set(ctx, "rbf", out, weights=((0.3, 0.7), (0.0, 1.0)))
    out["rbf/two_sets same it=3"] = _two_sets(ctx, ctx, (0.3, 0.7), 3)
    ctx.set_option("point_weight_evaluator", 0); ctx.set_option("plane_weight_evaluator", 0)
    # two sets: the same context twice, and two contexts with their own radius
    other = Context()
    other.share_target(ctx)
    other.set_source(S)
    out["found other"] = _bytes(np.uint64(other.find_correspondences(I4, 0.25 * r2)))
    for w in ((0.3, 0.7), (1.0, 0.0), (0.0, 1.0)):
        for it in (0, 3):
            out[f"two_sets same w={w[0]},{w[1]} it={it}"] = _two_sets(ctx, ctx, w, it)
            out[f"two_sets other w={w[0]},{w[1]} it={it}"] = _two_sets(ctx, other, w, it)
    res = capi.IcpResult()
    p = _params(ctx, r2, 3)
    ctx._ck(ctx._L.cilhip_icp_run_two_sets(ctx._h, C.c_float(r2), other._h, C.c_float(0.25 * r2), C.byref(p), None, C.byref(res)))
    out["icp_run_two_sets"] = _bytes(np.frombuffer(bytes(res), np.uint8))
    # a radius that leaves no correspondence
    out["found none"] = _bytes(np.uint64(ctx.find_correspondences(I4, 1e-14)))
    _single_set(ctx, "none", out, weights=((0.3, 0.7),), iters=(0, 1))
    out["none/two_sets it=0"] = _two_sets(ctx, ctx, (0.3, 0.7), 0)
    out["none/two_sets it=3"] = _two_sets(ctx, ctx, (0.3, 0.7), 3)
    other.close()
    # source normals: the symmetric objective
    ctx.set_source(S, SN)
    out["found sym"] = _bytes(np.uint64(ctx.find_correspondences(I4, r2)))
    _single_set(ctx, "sym", out, weights=((0.3, 0.7), (0.0, 1.0)), iters=(1, 5))
    # a pair-list direction (BOTH), with and without source normals
    ctx.set_option("search_direction", 2)
    out["found both sym"] = _bytes(np.uint64(ctx.find_correspondences(I4, r2)))
    _single_set(ctx, "both sym", out, weights=((0.3, 0.7),), iters=(0, 5))
    ctx.set_source(S)
    out["found both"] = _bytes(np.uint64(ctx.find_correspondences(I4, r2)))
    _single_set(ctx, "both", out, weights=((0.3, 0.7), (1.0, 0.0)), iters=(1, 5))
    ctx.set_option("search_direction", 0)
    # the affine classes' host-driven loop
    ctx.set_option("transform_mode", 1); ctx.set_option("affine_device_loop", 0)
    for metric in (capi.METRIC_COMBINED, capi.METRIC_POINT_TO_POINT):
        p = _params(ctx, r2, 3)
        p.metric = metric
        out[f"icp_run affine metric={metric}"] = _bytes(np.frombuffer(bytes(ctx.icp_run(p)), np.uint8))
    ctx.set_option("transform_mode", 0); ctx.set_option("affine_device_loop", 1)
    # sources of one point and of none
    for n in (1, 0):
        ctx.set_source(S[:n])
        out[f"found n={n}"] = _bytes(np.uint64(ctx.find_correspondences(I4, r2)))
        _single_set(ctx, f"n={n}", out, weights=((0.3, 0.7),), iters=(0, 1))
    ctx.close()
    if RECORD:
        np.savez_compressed(RECORD, **out)
    return out


def _compare(computed, select):
    want = np.load(RECORD or GOLDEN)
    names = [k for k in want.files if select(k)]
    assert names and sorted(k for k in computed if select(k)) == sorted(names)
    differ = [k for k in names if computed[k].tobytes() != want[k].tobytes()]
    assert not differ, differ


def test_the_fixture_covers_every_entry_and_case(computed):
    assert len(computed) >= 100
    for needle in ("unity/p2p", "unity/combined w=0.0,0.0 it=5", "unity/combined w=0.3,0.7 it=0", "rbf/combined w=0.3,0.7 it=5", "sym/combined w=0.0,1.0 it=1",
                   "both sym/combined w=0.3,0.7 it=5", "both/affine w=0.3,0.7 centered=1", "none/combined w=0.3,0.7 it=0", "n=1/p2p", "n=0/affine w=1.0,0.0 centered=0",
                   "two_sets same w=0.3,0.7 it=0", "two_sets other w=1.0,0.0 it=3", "icp_run_two_sets", "icp_run affine metric=0"):
        assert needle in computed, needle
    found = {k: int(np.frombuffer(computed[k].tobytes(), np.uint64)[0]) for k in computed if k.startswith("found")}
    assert found["found none"] == 0 and found["found n=0"] == 0 and found["found"] > 1000 and found["found both"] > 1000, found
    # (the estimates did estimate: a first Gauss-Newton step that is not the identity, normal equations that are not zero)
    step = np.frombuffer(computed["unity/combined w=0.3,0.7 it=1"].tobytes()[:64], np.float32)
    assert not np.array_equal(step, I4.reshape(16)) and np.frombuffer(computed["unity/combined w=0.3,0.7 it=1"].tobytes()[64:64 + 288], np.float64).any()


def test_single_set_estimates_are_bit_identical(computed):
    _compare(computed, lambda k: "/" in k and "two_sets" not in k)


def test_two_set_estimates_are_bit_identical(computed):
    _compare(computed, lambda k: "two_sets" in k and k != "icp_run_two_sets")


def test_host_driven_loops_and_counts_are_bit_identical(computed):
    _compare(computed, lambda k: k.startswith("icp_run") or k.startswith("found"))
