"""CPU: the two yardsticks of the mean-shift tests (tests/_meanshift_refs.py: the literal transcription of the reference's loop and the
restatement of the contract) against each other, the margins of the GPU fixtures, the parallel formulation of the grouping against the
serial first-fit, the argument rules of the C entry (they hold without a device), and the g++ build of the C++ mirror and the example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _meanshift_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("name", [f[0] for f in R.margin_fixtures()])
def test_literal_and_contract_agree_on_the_margin_fixtures(name):
    _, p, s, prm = next(f for f in R.margin_fixtures() if f[0] == name)
    a, b = R.cached("a", name), R.cached("b", name)
    assert np.array_equal(a["labels"], b["labels"]) and len(a["leaders"]) == len(b["leaders"]) and np.array_equal(a["offsets"], b["offsets"])
    # in (a) alone: no seed-leader distance between 0.9 and 1.1 cluster_tol
    assert R.leader_margin_ok(a["shifted"], a["leaders"], prm["cluster_tol"])
    gap = float(np.abs(a["shifted"].astype(np.float64) - b["shifted"].astype(np.float64)).max())
    print(f"{name}: passes a={a['iterations']} b={b['iterations']} sizes={np.diff(a['offsets']).tolist()} max|shifted_a - shifted_b|={gap:.3e}")
    assert gap <= R.RECORDED_GAP
    if name == "lattice":
        assert np.diff(a["offsets"]).tolist() == [150, 150, 150] and a["iterations"] == b["iterations"] == 6
    if name.startswith("lattice"):      # the exact-trajectory fixtures: on the 2^-10 lattice, inside (-8, 8), at most 2^16 points
        for arr in (p, s):
            if arr is not None:
                assert arr.shape[0] <= 1 << 16 and np.abs(arr).max() < 8 and np.array_equal(arr * 1024, np.round(arr * 1024))


def test_no_single_step_decision_is_within_4_ulp_of_the_radius():
    p = R.offset_cloud()
    seeds = p[::5] + np.float32(0.01)
    r2 = np.float32(0.4) * np.float32(0.4)
    assert R.ball_margin_ulps(seeds, p, r2) > 4 and R.ball_margin_ulps(p[::5], p, r2) > 4
    pop = (R.d2_pinned(seeds, p) < r2).sum(axis=1)
    assert pop.min() >= 1 and pop.max() > 20      # every ball holds a point; the sums are not trivial


def grouping_cases():
    rng = np.random.default_rng(8)
    dup = rng.random((150, 3)).astype(np.float32)
    dup = np.concatenate([dup, dup[:60], dup[:20]])[rng.permutation(230)]
    nan = R.collapsed_seeds(300)
    nan[[0, 7, 299]] = np.nan
    one = (np.array([0.3, 0.2, 10.0]) + (rng.random((1500, 3)) - 0.5) * 1e-6).astype(np.float32)      # the example's end state: every seed on one mode
    return [("one_mode", one, 0.2), ("chain", R.chain_seeds(200, 0.25), 0.25), ("chain_shuffled", R.chain_seeds(200, 0.25, shuffled=True), 0.25),
            ("uniform", rng.random((600, 3)).astype(np.float32), 0.15), ("collapsed", R.collapsed_seeds(), 0.01), ("duplicates", dup, 0.05),
            ("duplicates_tol0", dup, 0.0), ("nan_seeds", nan, 0.01)]


@pytest.mark.parametrize("name", [c[0] for c in grouping_cases()])
def test_rounds_formulation_equals_the_serial_first_fit(name):
    _, s, tol = next(c for c in grouping_cases() if c[0] == name)
    labels, leaders = R.first_fit(s, tol)
    got_labels, got_leaders, rounds = R.rounds_grouping(s, tol)
    assert np.array_equal(got_leaders, leaders) and np.array_equal(got_labels, labels)
    if name == "chain":
        assert len(leaders) == 100 and rounds == 100      # one round per leader: the worst case DESIGN.md 13.3 states
    if name == "collapsed":
        assert len(leaders) == 3 and rounds == 1
    if name == "uniform":
        assert 100 < len(leaders) < 600 and 1 < rounds < 30
    if name == "duplicates_tol0":
        assert len(leaders) == s.shape[0]      # d2 < 0 never holds: exact duplicates stay apart
    # stopped early, the formulation has decided a prefix of the leaders and nothing wrong
    for k in (1, 2, 4):
        _, part, _ = R.rounds_grouping(s, tol, max_rounds=k)
        fin = np.isfinite(s).all(axis=1)
        assert set(part.tolist()) - set(np.nonzero(~fin)[0].tolist()) <= set(leaders.tolist())


# ---- argument rules: before any device is opened ------------------------------------------------------------------------------
def call(L, n=4, ns=0, seeds=False, points=True, mem=0, params=True, outs=True, counts=(True, True), **fields):
    from cilantro_amd import capi

    pts = np.zeros((4, 3), np.float32)
    sd = np.zeros((4, 3), np.float32)
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol = 1.0, 5, 0.1
    for k, v in fields.items():
        setattr(prm, k, v)
    f = [np.full(15, 7, np.float32) for _ in range(2)]
    u = [np.full(5, 7, np.uint32) for _ in range(3)]
    nc, it = C.c_size_t(77), C.c_size_t(77)
    rc = L.cilhip_mean_shift3f(0, pts.ctypes.data if points else None, n, sd.ctypes.data if seeds else None, ns, mem, C.byref(prm) if params else None,
                               f[0].ctypes.data if outs else None, u[0].ctypes.data if outs else None, f[1].ctypes.data, u[1].ctypes.data, u[2].ctypes.data,
                               C.byref(nc) if counts[0] else None, C.byref(it) if counts[1] else None)
    untouched = all((a == 7).all() for a in f + u) and nc.value == 77 and it.value == 77
    return rc, untouched, L.cilhip_last_error(None).decode()


def test_refused_input_needs_no_device(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    nan, inf = float("nan"), float("inf")
    for kw, word in (({"points": False}, "points is null"), ({"ns": 3}, "seed array"), ({"n": 1 << 32}, "n must be below 2^32"), ({"seeds": True, "ns": 1 << 32}, "n_seeds must be below 2^32"),
                     ({"kernel_radius": nan}, "kernel_radius"), ({"kernel_radius": inf}, "kernel_radius"), ({"kernel_radius": -1.0}, "kernel_radius"),
                     ({"cluster_tol": nan}, "cluster_tol"), ({"cluster_tol": -0.5}, "cluster_tol"), ({"cluster_tol": inf}, "cluster_tol"),
                     ({"convergence_tol": nan}, "convergence_tol"), ({"convergence_tol": -1e-3}, "convergence_tol"), ({"convergence_tol": inf}, "convergence_tol"),
                     ({"kernel_kind": 2, "kernel_sigma": 0.0}, "kernel_sigma"), ({"kernel_kind": 2, "kernel_sigma": -1.0}, "kernel_sigma"), ({"kernel_kind": 2, "kernel_sigma": nan}, "kernel_sigma"),
                     ({"kernel_kind": 2, "kernel_sigma": inf}, "kernel_sigma"), ({"kernel_kind": 3}, "kernel_kind"), ({"kernel_kind": -1}, "kernel_kind"), ({"form": 3}, "form"),
                     ({"form": -1}, "form"), ({"mem": 2}, "mem"), ({"params": False}, "params is null"), ({"outs": False}, "shifted_seeds_out is null"),
                     ({"counts": (False, True)}, "n_clusters_out is null"), ({"counts": (True, False)}, "iterations_out is null")):
        rc, untouched, err = call(L, **kw)
        assert rc == capi.ERR_INVALID and untouched and word in err and err.startswith("mean_shift: "), (kw, rc, err)
    # a sigma is only looked at with the RBF kernel
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    assert (prm.kernel_kind, prm.form, prm.max_iter) == (0, 0, 0) and prm.convergence_tol == np.finfo(np.float32).eps and prm.kernel_sigma == 1.0
    # no seed at all: answered without a device -- an empty seed list, or every point a seed of an empty cloud
    for n, seeds in ((4, True), (0, False)):
        nc, it = C.c_size_t(77), C.c_size_t(77)
        off = np.full(1, 7, np.uint32)
        pts = np.zeros((4, 3), np.float32)
        prm.kernel_radius, prm.max_iter, prm.cluster_tol = 1.0, 5, 0.1
        rc = L.cilhip_mean_shift3f(0, pts.ctypes.data if n else None, n, pts.ctypes.data if seeds else None, 0, 0, C.byref(prm), None, None, None, off.ctypes.data, None,
                                   C.byref(nc), C.byref(it))
        assert rc == capi.OK and nc.value == 0 and it.value == 0 and off[0] == 0
    import torch

    if not torch.cuda.is_available():      # a valid call fails loudly: there is no CPU path
        rc, _, err = call(L)
        assert rc == capi.ERR_NO_DEVICE and "no CPU path" in err
        from cilantro_amd import clustering

        with pytest.raises(capi.CilhipError):
            clustering.MeanShift3f(np.zeros((4, 3), np.float32)).cluster(1.0, 5, 0.1)
        r = clustering.mean_shift(np.zeros((4, 3), np.float32), 1.0, 5, 0.1, seeds=np.zeros((0, 3), np.float32))
        assert r["labels"].shape == (0,) and r["offsets"].tolist() == [0] and r["iterations"] == 0


# ---- the C++ mirror and the example compile with g++ ----------------------------------------------------------------------------
def test_cpp_mirror_and_example_compile():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_mean_shift.cpp"), "test_mean_shift")
    build_cpp(os.path.join(ROOT, "examples", "mean_shift.cpp"), "example_mean_shift")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "mean_shift.cpp")).read()
    for needle in ("MeanShift3f<> ms", "ms.cluster(2.0f, 5000, 0.2f, 1e-7f, UnityWeightEvaluator<float>())", "getNumberOfPerformedIterations", "getClusterToPointIndicesMap"):
        assert needle in src, needle
