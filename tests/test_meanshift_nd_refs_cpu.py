"""CPU: the yardsticks of the N-D mean-shift tests (tests/_meanshift_nd_refs.py: the literal transcription of the reference's loop, the
restatement of rules M1-M7 and that restatement summed backwards) against each other and against the 3-D yardsticks, the margins of the
GPU fixtures, the parallel formulation of the grouping against the serial first-fit on N-D chains, the argument rules of
cilhip_mean_shift_nd (they hold without a device), csrc/mean_shift_nd_host.hpp stand-alone (plainly and under ASan / UBSan), and the g++
build of the C++ mirrors and the example."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _meanshift_nd_refs as R
import _meanshift_refs as R3

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _gap(a, b):
    return float(np.abs(a["shifted"].astype(np.float64) - b["shifted"].astype(np.float64)).max())


# ---- the fixtures' margins, the recorded gaps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", range(1, R.MAX_DIM + 1))
def test_lattice_fixtures_have_their_margins(dim):
    for name in (f"lattice_{dim}", f"lattice_seeds_{dim}"):
        _, p, s, prm = R.fixture(name)
        a, b, r = R.cached("a", name), R.cached("b", name), R.cached("r", name)
        assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["offsets"], b["offsets"]) and len(b["leaders"]) == 3
        assert R.leader_margin_ok(a["shifted"], a["leaders"], prm["cluster_tol"]) and R.leader_margin_ok(b["shifted"], b["leaders"], prm["cluster_tol"])
        assert 3 <= b["iterations"] <= 6 and a["iterations"] == b["iterations"] and np.isfinite(b["shifted"]).all()
        # on the 2^-10 lattice inside (-8, 8) with at most 2^16 points and the flat kernel every f64 sum is exact: no order exists
        for arr in (p, s):
            if arr is not None:
                assert arr.shape[0] <= 1 << 16 and np.abs(arr).max() < 8 and np.array_equal(arr * 1024, np.round(arr * 1024)) and arr.shape[1] == dim
        assert b["shifted"].tobytes() == r["shifted"].tobytes() and b["modes"].tobytes() == r["modes"].tobytes() and b["iterations"] == r["iterations"]
        print(f"{name}: passes {b['iterations']} sizes {np.diff(b['offsets']).tolist()} max|literal - contract| = {_gap(a, b):.3e}")
        assert _gap(a, b) <= R.RECORDED_GAP_ND
    assert np.diff(R.cached("b", f"lattice_{dim}")["offsets"]).tolist() == [60, 60, 60]


@pytest.mark.parametrize("dim", R.UNIT_DIMS)
def test_unit_fixtures_have_their_margins_and_the_recorded_gaps_hold(dim):
    name = f"unit_{dim}"
    _, p, s, prm = R.fixture(name)
    a, b, r = R.cached("a", name), R.cached("b", name), R.cached("r", name)
    assert np.array_equal(a["labels"], b["labels"]) and np.array_equal(a["labels"], r["labels"]) and np.array_equal(a["offsets"], b["offsets"])
    for x in (a, b, r):
        assert R.leader_margin_ok(x["shifted"], x["leaders"], prm["cluster_tol"])
    gap, order_gap = _gap(a, b), _gap(b, r)
    print(f"{name}: passes literal {a['iterations']} contract {b['iterations']} clusters {len(b['leaders'])} max|literal - contract| = {gap:.3e} "
          f"max|contract - reversed| = {order_gap:.3e}")
    assert gap <= R.RECORDED_GAP_ND and order_gap <= R.RECORDED_ORDER_GAP_ND
    assert len(b["leaders"]) >= 2 and b["iterations"] > 3


def single_step_cases():
    """(dim, kind, sigma, points, seeds, radius) of the single-step fixtures"""
    out = []
    for dim in (2, 6, 16):
        p = R.offset_cloud_nd(dim)
        seeds = np.ascontiguousarray(p[::5] + np.float32(0.01))
        for kind, sigma in ((R.IDENTITY, 1.0), (R.RBF, 0.15)):
            out.append((dim, kind, sigma, p, seeds, np.float32(0.4)))
    return out


def test_no_single_step_decision_is_within_4_ulp_of_the_radius():
    for dim, _, _, p, seeds, radius in single_step_cases()[::2]:
        r2 = radius * radius
        assert R.ball_margin_ulps(seeds, p, r2) > 4, dim
        pop = (R.d2_rows(seeds, p) < r2).sum(axis=1)
        print("dim", dim, "ball populations", int(pop.min()), "to", int(pop.max()))
        assert pop.min() >= 1 and pop.max() > 20 and abs(p).min() > 90      # every ball holds a point; the sums are not trivial; far from the origin


# ---- the restatements against the 3-D ones --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "lattice_seeds", "unit"])
def test_contract_nd_at_dim_3_is_the_3d_contract(name):
    _, p, s, prm = next(f for f in R3.margin_fixtures() if f[0] == name)
    want = R3.cached("b", name)
    got = R.contract_nd(p, s, **prm)
    for k in ("shifted", "modes"):
        assert got[k].tobytes() == want[k].tobytes(), k
    for k in ("labels", "offsets", "members", "leaders"):
        assert np.array_equal(got[k], want[k]), k
    assert got["iterations"] == want["iterations"] and set(got["slices"]) == {1}
    lit = R.literal_nd(p, s, **prm)
    assert lit["shifted"].tobytes() == R3.cached("a", name)["shifted"].tobytes() and lit["iterations"] == R3.cached("a", name)["iterations"]


def test_the_slice_plan_is_part_of_the_contract():
    """with more than one slice the f64 sums are taken slice by slice; on an unquantised cloud the restatement follows the plan"""
    src = open(os.path.join(ROOT, "cilantro_amd", "csrc", "mean_shift_nd_host.hpp")).read()
    m = re.search(r"MSN_TARGET_BLOCKS = (\d+), MSN_MIN_SLICE = MSN_MIN_SLICE_POINTS, MSN_MAX_SLICES = MSN_SLICE_CAP, MSN_PART_BYTES = \(size_t\)(\d+) << 20;", src)
    assert m and tuple(int(g) for g in m.groups()) == (R.TARGET_BLOCKS, R.PART_BYTES >> 20)
    assert f"#define MSN_MIN_SLICE_POINTS {R.MIN_SLICE}\n" in src and f"#define MSN_SLICE_CAP {R.MAX_SLICES}\n" in src
    assert re.search(r"constexpr size_t MSN_TILE = (\d+);", src).group(1) == str(R.TILE)
    assert R.msn_slices(4097, 41) == 8 and R.msn_slices(1025, 257) == 2 and R.msn_slices(1023, 41) == 1 and R.msn_slices(1 << 20, 10000) == 26
    assert R.msn_slice_length(4097, 8) == 516 and R.msn_slice_length(5, 1) == 8
    p = R.unit_blobs_nd(6, per=400)
    seeds = p[::40]
    one = R.contract_nd(p, seeds, max_iter=2, kernel_radius=2.0, cluster_tol=0.2)
    assert set(one["slices"]) == {2}      # 1200 points, 30 seeds
    back = R.contract_nd(p, seeds, max_iter=2, kernel_radius=2.0, cluster_tol=0.2, reverse=True)
    # (the two orders' f64 sums differ by at most a few 2^-53: the f32 roundings of a pass can differ in the last bit only, half an ulp of 16 each way)
    assert np.abs(one["shifted"].astype(np.float64) - back["shifted"].astype(np.float64)).max() <= 2 * 2.0 ** -20


@pytest.mark.parametrize("dim", [1, 5, 16])
def test_the_matrix_product_form_is_the_contract_on_the_lattice(dim):
    cloud = R.lattice_cloud_nd(dim, 1300, 70 + dim)
    cloud[17, 0], cloud[400, dim - 1] = np.nan, np.inf      # non-finite rows are in no ball
    seeds = np.concatenate([R.lattice_seeds_nd(dim), R.quantise(np.full((1, dim), -7.5))])      # the last one finds nothing
    prm = dict(R.LATTICE, max_iter=20)
    for p, s in ((R.lattice_blobs_nd(dim), None), (cloud, seeds)):
        want, got = R.contract_nd(p, s, **prm), R.contract_lattice(p, s, **prm)
        for k in ("shifted", "modes"):
            assert got[k].tobytes() == want[k].tobytes(), k
        for k in ("labels", "offsets", "members"):
            assert np.array_equal(got[k], want[k]), k
        assert got["iterations"] == want["iterations"] and got["slices"] == want["slices"]
    assert want["iterations"] == 20 and np.isnan(want["shifted"][-1]).all() and set(want["slices"]) == {2}


# ---- the grouping ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 6, 9, 16])
def test_rounds_formulation_equals_the_serial_first_fit_in_n_dimensions(dim):
    for name, s, tol in R.grouping_cases(dim):
        labels, leaders = R.first_fit(s, tol)
        got_labels, got_leaders, rounds = R.rounds_grouping(s, tol)
        assert np.array_equal(got_leaders, leaders) and np.array_equal(got_labels, labels), (dim, name)
        if name == "chain":
            assert len(leaders) == 100 and rounds == 100      # one round per leader: the worst case DESIGN.md 22.4 states
        if name == "chain_shuffled":
            assert len(leaders) < 200 and rounds > 1
        if name == "collapsed":
            assert len(leaders) == 3 and rounds == 1
        if name == "duplicates_tol0":
            assert len(leaders) == s.shape[0]      # d2 < 0 never holds: exact duplicates stay apart
        if name == "nan_seeds":
            assert len(leaders) == 3 + 3 and set([0, 7, 299]) <= set(leaders.tolist())


# ---- argument rules: before any device is opened ------------------------------------------------------------------------------
def call(L, n=4, dim=5, ns=0, seeds=False, points=True, mem=0, params=True, outs=(True, True), counts=(True, True), **fields):
    from cilantro_amd import capi

    pts = np.zeros((4, 20), np.float32)
    sd = np.zeros((4, 20), np.float32)
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol = 1.0, 5, 0.1
    for k, v in fields.items():
        setattr(prm, k, v)
    f = [np.full(100, 7, np.float32) for _ in range(2)]
    u = [np.full(5, 7, np.uint32) for _ in range(3)]
    nc, it = C.c_size_t(77), C.c_size_t(77)
    rc = L.cilhip_mean_shift_nd(0, pts.ctypes.data if points else None, n, dim, sd.ctypes.data if seeds else None, ns, mem, C.byref(prm) if params else None,
                                f[0].ctypes.data if outs[0] else None, u[0].ctypes.data if outs[1] else None, f[1].ctypes.data, u[1].ctypes.data, u[2].ctypes.data,
                                C.byref(nc) if counts[0] else None, C.byref(it) if counts[1] else None)
    untouched = all((a == 7).all() for a in f + u) and nc.value == 77 and it.value == 77
    return rc, untouched, L.cilhip_last_error(None).decode()


def test_refused_input_needs_no_device(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    nan, inf = float("nan"), float("inf")
    rows = [({"dim": 0}, "dim is 0"), ({"form": 1}, "form must be 0"), ({"form": 2}, "form must be 0"), ({"form": -1}, "form must be 0"),
            ({"n": 2 ** 32 - 16}, "n must be below 2^32 - 16"), ({"seeds": True, "ns": 2 ** 32 - 16}, "n_seeds must be below 2^32 - 16"),
            ({"points": False}, "points is null"), ({"ns": 3}, "seed array"),
            ({"kernel_radius": nan}, "kernel_radius"), ({"kernel_radius": inf}, "kernel_radius"), ({"kernel_radius": -1.0}, "kernel_radius"),
            ({"cluster_tol": nan}, "cluster_tol"), ({"cluster_tol": -0.5}, "cluster_tol"), ({"cluster_tol": inf}, "cluster_tol"),
            ({"convergence_tol": nan}, "convergence_tol"), ({"convergence_tol": -1e-3}, "convergence_tol"), ({"convergence_tol": inf}, "convergence_tol"),
            ({"kernel_kind": 2, "kernel_sigma": 0.0}, "kernel_sigma"), ({"kernel_kind": 2, "kernel_sigma": -1.0}, "kernel_sigma"), ({"kernel_kind": 2, "kernel_sigma": nan}, "kernel_sigma"),
            ({"kernel_kind": 2, "kernel_sigma": inf}, "kernel_sigma"), ({"kernel_kind": 3}, "kernel_kind"), ({"kernel_kind": -1}, "kernel_kind"),
            ({"mem": 2}, "mem"), ({"mem": -1}, "mem"), ({"params": False}, "params is null"), ({"outs": (False, True)}, "shifted_seeds_out is null"),
            ({"outs": (True, False)}, "labels_out is null"), ({"counts": (False, True)}, "n_clusters_out is null"), ({"counts": (True, False)}, "iterations_out is null")]
    for kw, word in rows:
        rc, untouched, err = call(L, **kw)
        assert rc == capi.ERR_INVALID and untouched and word in err and err.startswith("mean_shift_nd: "), (kw, rc, err)
    for dim in (17, 1000):
        rc, untouched, err = call(L, dim=dim)
        assert rc == capi.ERR_UNSUPPORTED and untouched and "dim > 16" in err and err.startswith("mean_shift_nd: "), (dim, rc, err)
    # no seed at all: answered without a device -- an empty seed list, or every point a seed of an empty cloud
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol = 1.0, 5, 0.1
    for n, seeds in ((4, True), (0, False)):
        nc, it = C.c_size_t(77), C.c_size_t(77)
        off = np.full(1, 7, np.uint32)
        pts = np.zeros((4, 6), np.float32)
        rc = L.cilhip_mean_shift_nd(0, pts.ctypes.data if n else None, n, 6, pts.ctypes.data if seeds else None, 0, 0, C.byref(prm), None, None, None, off.ctypes.data, None,
                                    C.byref(nc), C.byref(it))
        assert rc == capi.OK and nc.value == 0 and it.value == 0 and off[0] == 0
    from cilantro_amd import clustering

    r = clustering.mean_shift_nd(np.zeros((4, 9), np.float32), 1.0, 5, 0.1, seeds=np.zeros((0, 9), np.float32))
    assert r["labels"].shape == (0,) and r["offsets"].tolist() == [0] and r["iterations"] == 0 and r["shifted"].shape == (0, 9) and r["modes"].shape == (0, 9) and r["stats"] == {}
    ms = clustering.MeanShiftXf(np.zeros((0, 4), np.float32)).cluster(1.0, 5, 0.1)
    assert ms.getNumberOfClusters() == 0 and ms.getNumberOfPerformedIterations() == 0 and ms.dim == 4
    with pytest.raises(capi.CilhipError) as e:
        clustering.MeanShiftXf(np.zeros((4, 17), np.float32)).cluster(1.0, 5, 0.1)
    assert e.value.code == capi.ERR_UNSUPPORTED and "dim > 16" in str(e.value)
    with pytest.raises(ValueError):
        clustering.MeanShift2f(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        clustering.MeanShiftXf(np.zeros((4, 3), np.float32), dim=4)
    with pytest.raises(ValueError):
        clustering.mean_shift_nd(np.zeros((4, 3), np.float32), 1.0, 5, 0.1, seeds=np.zeros((2, 4), np.float32))
    import torch

    if not torch.cuda.is_available():      # a valid call fails loudly: there is no CPU path
        rc, _, err = call(L)
        assert rc == capi.ERR_NO_DEVICE and "no CPU path" in err
        with pytest.raises(capi.CilhipError):
            clustering.MeanShift2f(np.zeros((4, 2), np.float32)).cluster(1.0, 5, 0.1)


def test_symbols_sources_and_exports():
    import cilantro_amd
    from cilantro_amd import build, capi, clustering

    header = open(os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")).read()
    for sym in ("cilhip_mean_shift_nd", "cilhip_msn_last_stats"):
        assert sym in capi.SYMBOLS and re.search(r"\bint " + sym + r"\(", header), sym
    assert "typedef struct cilhip_msn_stats { size_t passes, rounds, slices_first, slices_last; double shift_ms, group_ms; } cilhip_msn_stats;" in header
    assert [f[0] for f in capi.MsnStats._fields_] == ["passes", "rounds", "slices_first", "slices_last", "shift_ms", "group_ms"]
    for rule in ("M1 ball", "M2 weights", "M3 step", "M4 converged", "M5 empty", "M6 grouping", "M7 modes"):
        assert rule in header, rule
    assert "mean_shift_nd.hip" in build.SOURCES and "mean_shift_nd_host.hpp" in build.HEADERS and "nd_device.hpp" in build.HEADERS
    host = open(os.path.join(ROOT, "cilantro_amd", "csrc", "mean_shift_nd_host.hpp")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host      # plain C++
    unit = open(os.path.join(ROOT, "cilantro_amd", "csrc", "mean_shift_nd.hip")).read()
    assert "atomic" not in unit.replace("no atomics", "").replace("floating-point atomics", "")      # M3, M6: nothing is accumulated or claimed by an atomic
    for name in ("MeanShift3f", "MeanShift2f", "MeanShiftXf", "mean_shift", "mean_shift_nd"):
        assert getattr(cilantro_amd, name) is getattr(clustering, name) and name in cilantro_amd.__all__
    assert issubclass(clustering.MeanShift2f, clustering.MeanShiftXf)
    for method in ("cluster", "getShiftedSeeds", "getClusterModes", "getNumberOfPerformedIterations", "getPointToClusterIndexMap", "getNumberOfClusters", "getClusterToPointIndicesMap"):
        assert callable(getattr(clustering.MeanShiftXf, method))


# ---- mean_shift_nd_host.hpp on its own, the C++ mirrors and the example -------------------------------------------------------------
def test_host_header_stand_alone_plain_and_sanitized(tmp_path):
    src = os.path.join(HERE, "cpp", "test_mean_shift_nd_host.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_mean_shift_nd_host_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr[-2000:]


def test_cpp_mirrors_and_example_compile():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_mean_shift_nd.cpp"), "test_mean_shift_nd")
    build_cpp(os.path.join(ROOT, "examples", "mean_shift_nd.cpp"), "example_mean_shift_nd")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "mean_shift_nd.cpp")).read()
    for needle in ("MeanShiftXf<> ms{ConstDataView(features, dim)}", "ms.cluster(2.0f, 5000, 0.2f, 1e-7f, UnityWeightEvaluator<float>())", "getNumberOfPerformedIterations",
                   "getClusterToPointIndicesMap"):
        assert needle in src, needle
    mirror = open(os.path.join(ROOT, "include", "cilantro_hip", "clustering.hpp")).read()
    assert "class MeanShiftXf" in mirror and "class MeanShift2f" in mirror and "class MeanShift3f" in mirror
