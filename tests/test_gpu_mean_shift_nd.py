"""GPU: mean-shift clustering in 1 to 16 dimensions (cilhip_mean_shift_nd and its Python / C++ mirrors) against the numpy yardsticks of
tests/_meanshift_nd_refs.py (pinned on the CPU by tests/test_meanshift_nd_refs_cpu.py, which also asserts the margins these fixtures
need).  On the 2^-10 lattice with the flat kernel every f64 sum is exact in any order, so whole trajectories are compared with
np.array_equal; elsewhere the bounds are the derived ones of DESIGN.md sections 13.2 and 22."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _meanshift_nd_refs as R
import _meanshift_refs as R3

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = ("shifted", "labels", "offsets", "members")


@pytest.fixture(scope="module")
def cl():
    from cilantro_amd import clustering

    return clustering


def evaluator(cl, kind, sigma=1.0):
    return (cl.UnityWeightEvaluator(), cl.IdentityWeightEvaluator(), cl.RBFKernelWeightEvaluator(sigma))[kind]


def run(cl, points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(np.float32).eps, kind=0, sigma=1.0, device_mem=False):
    """one call -> the result with every array as numpy"""
    if device_mem:
        import torch

        points = torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()
        seeds = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, np.float32)).cuda()
    r = cl.mean_shift_nd(points, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator(cl, kind, sigma), seeds=seeds)
    if device_mem:
        assert all(r[k].is_cuda for k in EXACT + ("modes",))
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    return r


def same(got, want, what=EXACT):
    for k in what:
        assert np.array_equal(got[k], want[k], equal_nan=(k in ("shifted", "modes"))), k
    assert got["iterations"] == want["iterations"], (got["iterations"], want["iterations"])


# ---- exact trajectory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", range(1, R.MAX_DIM + 1))
def test_exact_trajectory_on_the_lattice(cl, dim):
    for name in (f"lattice_{dim}", f"lattice_seeds_{dim}"):
        _, p, s, prm = R.fixture(name)
        want = R.cached("b", name)
        assert 3 <= want["iterations"] <= 6 and len(want["leaders"]) == 3
        for device_mem in (False, True):
            got = run(cl, p, s, device_mem=device_mem, **prm)
            same(got, want, EXACT + ("modes",))      # (a lattice mode's f64 sum is exact too)
            assert got["shifted"].shape == (len(want["labels"]), dim) and got["modes"].shape == (3, dim)
            assert got["stats"]["passes"] == want["iterations"] and got["stats"]["rounds"] >= 1 and got["stats"]["slices_first"] == got["stats"]["slices_last"] == 1
            assert np.array_equal(got["members"][got["offsets"][:-1]], want["leaders"])      # a cluster's first member is its leader


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
SIZE_PRM = dict(R.LATTICE, max_iter=12)


@pytest.mark.parametrize("dim", [5, 6, 7, 9, 16])
def test_point_counts_around_the_tile_and_the_slice_edges(cl, dim):
    seeds = R.lattice_seeds_nd(dim)      # 41 seeds
    for n in (1, 2, 3, 4, 5, 511, 512, 513, 1025, 4097):
        p = R.lattice_cloud_nd(dim, n, 100 * dim + n % 97)
        want = R.contract_lattice(p, seeds, **SIZE_PRM)
        got = run(cl, p, seeds, **SIZE_PRM)
        same(got, want, EXACT + ("modes",))
        plan = R.msn_slices(n, 41)
        assert got["stats"]["slices_first"] == plan == want["slices"][0] and (plan > 1) == (n >= 1024), (n, plan)
        assert got["stats"]["slices_last"] == want["slices"][-1] and got["stats"]["passes"] == len(want["slices"])
    assert R.msn_slices(4097, 41) == 8 and R.msn_slice_length(4097, 8) % R.TILE == 0 and 7 * R.msn_slice_length(4097, 8) < 4097      # eight slices, the last one short


@pytest.mark.parametrize("dim", [5, 6, 7, 9, 16])
def test_seed_counts_around_the_wave_and_the_block_edges(cl, dim):
    p = R.lattice_cloud_nd(dim, 1100, 7 * dim)
    for ns in (1, 63, 64, 65, 255, 256, 257):
        seeds = R.lattice_seeds_nd(dim, n=ns, seed=300 + ns)
        want = R.contract_lattice(p, seeds, **SIZE_PRM)
        for device_mem in (False, True):
            got = run(cl, p, seeds, device_mem=device_mem, **SIZE_PRM)
            same(got, want, EXACT + ("modes",))
            assert got["stats"]["slices_first"] == want["slices"][0] == 2


def test_the_slice_count_changes_when_the_active_count_crosses_a_block_boundary(cl):
    """106 000 points, 1100 seeds: five blocks of seeds give 205 slices; after the first pass the 100 seeds that found nothing are NaN, four
    blocks are left and the plan says 207.  On the lattice the sums are exact under either plan."""
    dim = 5
    p = R.lattice_cloud_nd(dim, 106000, 11)[: 1 << 16]      # (at most 2^16 points keep every sum exact) ...
    p = np.concatenate([p, np.full((106000 - p.shape[0], dim), np.nan, np.float32)])      # ... the rest of the stream is in no ball
    seeds = np.concatenate([R.lattice_seeds_nd(dim, n=1000, seed=12), R.quantise(np.full((100, dim), -7.5))])[np.random.default_rng(13).permutation(1100)]
    prm = dict(R.LATTICE, max_iter=2)
    want = R.contract_lattice(p, seeds, **prm)
    assert want["slices"] == [205, 207] and int(np.isnan(want["shifted"][:, 0]).sum()) == 100
    got = run(cl, p, seeds, **prm)
    same(got, want)
    assert (got["stats"]["slices_first"], got["stats"]["slices_last"], got["stats"]["passes"]) == (205, 207, 2)


# ---- dim = 3: the 3-D entry's results ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lattice", "lattice_seeds"])
def test_dim_3_equals_the_3d_entry(cl, name):
    _, p, s, prm = next(f for f in R3.margin_fixtures() if f[0] == name)
    for device_mem in (False, True):
        if device_mem:
            import torch

            dp, ds = torch.from_numpy(p).cuda(), None if s is None else torch.from_numpy(s).cuda()
        else:
            dp, ds = p, s
        old = cl.mean_shift(dp, prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"], seeds=ds)
        new = cl.mean_shift_nd(dp, prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"], seeds=ds)
        for k in EXACT + ("modes",):
            a, b = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (old[k], new[k]))
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), k
        assert old["iterations"] == new["iterations"] == 6


# ---- single step: derived bound against the exact rational mean ----------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 6, 16])
@pytest.mark.parametrize("kind,sigma", [(R.IDENTITY, 1.0), (R.RBF, 0.15)])
def test_single_step_is_within_the_derived_bound(cl, dim, kind, sigma):
    from test_meanshift_nd_refs_cpu import single_step_cases

    _, _, _, p, seeds, radius = next(c for c in single_step_cases() if c[0] == dim and c[1] == kind)
    seeds = seeds[::2]
    r2 = radius * radius
    exact = [R.exact_step_nd(s, p, r2, kind, sigma) for s in seeds]
    m, bound = np.array([e[0] for e in exact]), np.array([e[1] for e in exact])
    assert max(e[2] for e in exact) > 20
    got = run(cl, p, seeds, radius, 1, 0.05, kind=kind, sigma=sigma)
    err = np.abs(got["shifted"].astype(np.float64) - m)
    print(f"dim {dim} kind {kind}: max err / bound = {(err / bound).max():.3f}, largest error {err.max():.3e}")
    assert got["iterations"] == 1 and (err <= bound).all()


# ---- grouping alone (max_iter = 0): exact against the serial first-fit ---------------------------------------------------------------
def grouping_check(cl, seeds, tol):
    dim = seeds.shape[1]
    labels, leaders = R.first_fit(seeds, tol)
    offsets, members = R3.lists_of(labels, len(leaders))
    got = run(cl, np.zeros((3, dim), np.float32), seeds, 1.0, 0, tol)
    assert got["iterations"] == 0 and got["shifted"].tobytes() == seeds.tobytes()      # bit for bit, NaN payloads included
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["offsets"], offsets) and np.array_equal(got["members"], members)
    assert np.array_equal(got["members"][got["offsets"][:-1]], leaders)
    return got, leaders


@pytest.mark.parametrize("dim", [1, 2, 6, 9, 16])
def test_grouping_equals_the_serial_first_fit(cl, dim):
    for name, seeds, tol in R.grouping_cases(dim):
        got, leaders = grouping_check(cl, seeds, tol)
        if name == "chain":      # one round per leader, and it finishes
            assert len(leaders) == 100 and got["stats"]["rounds"] == 100
        if name == "chain_shuffled":
            assert got["stats"]["rounds"] == R.rounds_grouping(seeds, tol)[2] > 1
        if name == "collapsed":
            assert len(leaders) == 3 and got["stats"]["rounds"] == 1 and sorted(np.diff(got["offsets"]).tolist())[0] > 600
        if name == "duplicates_tol0":      # answered without a round
            assert len(leaders) == seeds.shape[0] and got["stats"]["rounds"] == 0
        if name == "nan_seeds":
            assert all(np.diff(got["offsets"])[got["labels"][i]] == 1 for i in (0, 7, 299))


# ---- modes ------------------------------------------------------------------------------------------------------------------------------
def test_modes_are_within_the_derived_bound_of_the_exact_member_mean(cl):
    _, p, s, prm = R.fixture("unit_6")
    runs = [run(cl, p, s, **prm), run(cl, np.zeros((3, 9), np.float32), R.collapsed_seeds_nd(9), 1.0, 0, 0.01)]
    for got in runs:
        k = len(got["offsets"]) - 1
        assert got["modes"].shape == (k, got["shifted"].shape[1]) and k >= 2
        for c in range(k):
            m, bound = R.exact_mode_nd(got["shifted"], got["members"][got["offsets"][c]:got["offsets"][c + 1]])
            assert (np.abs(got["modes"][c].astype(np.float64) - m) <= bound).all(), c


# ---- edge rules -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 6, 16])
def test_empty_ball_becomes_a_nan_singleton_and_the_count_is_max_iter(cl, dim):
    p = R.lattice_blobs_nd(dim)
    seeds = np.concatenate([R.lattice_seeds_nd(dim)[:10], R.quantise(np.full((1, dim), -7.5)), R.lattice_seeds_nd(dim)[10:20]])
    prm = dict(R.LATTICE, max_iter=40)
    want = R.contract_nd(p, seeds, **prm)
    assert want["iterations"] == 40 and np.isnan(want["shifted"][10]).all() and np.isfinite(np.delete(want["shifted"], 10, axis=0)).all()
    got = run(cl, p, seeds, **prm)
    same(got, want)
    c = got["labels"][10]
    assert got["stats"]["passes"] < 40 and np.diff(got["offsets"])[c] == 1 and np.isnan(got["modes"][c]).all() and np.isfinite(np.delete(got["modes"], c, axis=0)).all()


@pytest.mark.parametrize("dim", [2, 6, 16])
def test_non_finite_seeds_and_points(cl, dim):
    p = R.lattice_blobs_nd(dim)
    seeds = R.lattice_seeds_nd(dim).copy()
    seeds[3, dim - 1], seeds[17, 0], seeds[40] = np.nan, np.inf, -np.inf
    want = R.contract_nd(p, seeds, **R.LATTICE)
    assert want["iterations"] == R.LATTICE["max_iter"] and np.isnan(want["shifted"][[3, 17, 40]]).all()
    same(run(cl, p, seeds, **R.LATTICE), want)
    # NaN / inf data points are in no ball: the others see the cloud without those rows
    rng = np.random.default_rng(9)
    bad = rng.permutation(p.shape[0])[:30]
    q = p.copy()
    q[bad[:10], 0], q[bad[10:20], dim - 1], q[bad[20:], dim // 2] = np.nan, np.inf, -np.inf
    q[-1] = np.nan
    clean = q[np.isfinite(q).all(axis=1)]
    good_seeds = R.lattice_seeds_nd(dim)
    want = R.contract_nd(clean, good_seeds, **R.LATTICE)
    for device_mem in (False, True):
        same(run(cl, q, good_seeds, device_mem=device_mem, **R.LATTICE), want)
    # ... and with every point a seed, the non-finite rows are NaN singletons and the rest is what the clean cloud's seeds do
    got = run(cl, q, None, **R.LATTICE)
    ok = np.isfinite(q).all(axis=1)
    ref = R.contract_nd(clean, None, **dict(R.LATTICE, max_iter=got["stats"]["passes"]))
    assert got["iterations"] == R.LATTICE["max_iter"] and np.array_equal(got["shifted"][ok], ref["shifted"]) and np.isnan(got["shifted"][~ok]).all()
    assert len(got["offsets"]) - 1 == len(ref["leaders"]) + int((~ok).sum())


def test_no_points_a_zero_radius_and_one_pass(cl):
    dim = 7
    seeds = R.lattice_seeds_nd(dim)[:9]
    got = run(cl, np.zeros((0, dim), np.float32), seeds, 1.0, 7, 0.25)
    assert got["iterations"] == 7 and got["stats"]["passes"] == 1 and np.isnan(got["shifted"]).all() and np.array_equal(got["labels"], np.arange(9))
    assert np.array_equal(got["offsets"], np.arange(10)) and np.array_equal(got["members"], np.arange(9)) and np.isnan(got["modes"]).all()
    got = run(cl, np.zeros((0, dim), np.float32), seeds, 1.0, 0, 0.25)      # no pass: the seeds as they came, grouped
    assert got["iterations"] == 0 and np.array_equal(got["shifted"], seeds)
    p = R.lattice_blobs_nd(dim)
    got = run(cl, p, p[:9].copy(), 0.0, 5, 0.25)      # d2 < 0 never holds, not even for a seed on a point
    assert got["iterations"] == 5 and got["stats"]["passes"] == 1 and np.isnan(got["shifted"]).all()
    prm = dict(R.LATTICE, max_iter=1)
    want = R.contract_nd(p, None, **prm)
    assert want["iterations"] == 1 and len(want["leaders"]) > 3      # not converged: more clusters than modes
    same(run(cl, p, None, **prm), want)


def test_rbf_weights_below_the_cut_give_the_nan_rule(cl):
    from oracle import oracle as orc

    dim = 6
    p = R.lattice_blobs_nd(dim)
    seeds = (R.lattice_seeds_nd(dim)[:12] + np.float32(2.0 ** -11)).astype(np.float32)      # half a lattice step off every point
    sigma = 1e-5
    d2 = R.d2_rows(seeds, p)
    inside = d2 < np.float32(1.0)
    assert inside.any(axis=1).all() and (R3.rbf_coeff(sigma) * d2[inside] < -80).all() and not orc.pinned_expf(R3.rbf_coeff(sigma) * d2[inside]).any()
    got = run(cl, p, seeds, 1.0, 5, 0.25, kind=R.RBF, sigma=sigma)
    assert got["iterations"] == 5 and got["stats"]["passes"] == 1 and np.isnan(got["shifted"]).all() and np.array_equal(got["labels"], np.arange(12))


def test_optional_outputs_may_be_null(cl):
    """modes, offsets and members are optional, each on its own, in host and in device memory; what is asked for does not change"""
    import torch

    from cilantro_amd import capi

    L = capi.load()
    dim = 6
    _, p, _, prm_d = R.fixture(f"lattice_{dim}")
    want = R.cached("b", f"lattice_{dim}")
    ns = p.shape[0]
    prm = capi.MsParams()
    L.cilhip_ms_default_params(C.byref(prm))
    prm.kernel_radius, prm.max_iter, prm.cluster_tol, prm.convergence_tol = prm_d["kernel_radius"], prm_d["max_iter"], prm_d["cluster_tol"], prm_d["convergence_tol"]
    dp = torch.from_numpy(p).cuda()
    for mem in (capi.MEM_HOST, capi.MEM_DEVICE):
        for ask in ((), ("modes",), ("offsets",), ("members",), ("offsets", "members"), ("modes", "offsets", "members")):
            if mem == capi.MEM_HOST:
                out = {"shifted": np.full((ns, dim), 7, np.float32), "labels": np.full(ns, 7, np.uint32), "modes": np.full((ns, dim), 7, np.float32),
                       "offsets": np.full(ns + 1, 7, np.uint32), "members": np.full(ns, 7, np.uint32)}
                addr = {k: v.ctypes.data for k, v in out.items()}
                src = p.ctypes.data
            else:
                out = {"shifted": torch.full((ns, dim), 7.0, device="cuda"), "labels": torch.full((ns,), 7, dtype=torch.int32, device="cuda"),
                       "modes": torch.full((ns, dim), 7.0, device="cuda"), "offsets": torch.full((ns + 1,), 7, dtype=torch.int32, device="cuda"),
                       "members": torch.full((ns,), 7, dtype=torch.int32, device="cuda")}
                addr = {k: v.data_ptr() for k, v in out.items()}
                src = dp.data_ptr()
                torch.cuda.synchronize()
            nc, it = C.c_size_t(0), C.c_size_t(0)
            rc = L.cilhip_mean_shift_nd(0, src, ns, dim, None, 0, mem, C.byref(prm), addr["shifted"], addr["labels"], *(addr[k] if k in ask else None for k in ("modes", "offsets", "members")),
                                        C.byref(nc), C.byref(it))
            assert rc == capi.OK, L.cilhip_last_error(None).decode()
            host = {k: (v if mem == capi.MEM_HOST else v.cpu().numpy()) for k, v in out.items()}
            assert nc.value == 3 and it.value == want["iterations"] and np.array_equal(host["shifted"], want["shifted"]) and np.array_equal(host["labels"], want["labels"])
            for k in ("modes", "offsets", "members"):
                if k in ask:
                    assert np.array_equal(host[k][: len(want[k])], want[k]), (mem, ask, k)
                else:
                    assert (host[k] == 7).all(), (mem, ask, k)


# ---- end to end against the literal transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", R.UNIT_DIMS)
def test_end_to_end_against_the_literal_transcription(cl, dim):
    name = f"unit_{dim}"
    _, p, s, prm = R.fixture(name)
    a = R.cached("a", name)
    # the literal-contract gap twice (the device's own summation order gets one more of it) plus the contract's own order gap, both measured
    # between the CPU restatements alone (test_meanshift_nd_refs_cpu.py)
    bound = 2.0 * R.RECORDED_GAP_ND + R.RECORDED_ORDER_GAP_ND
    for device_mem in (False, True):
        got = run(cl, p, s, device_mem=device_mem, **prm)
        assert np.array_equal(got["labels"], a["labels"]) and len(got["offsets"]) - 1 == len(a["leaders"])
        gap = float(np.abs(got["shifted"].astype(np.float64) - a["shifted"].astype(np.float64)).max())
        print(f"{name}: passes {got['iterations']} (literal {a['iterations']}), max |shifted - literal| = {gap:.3e}, bound {bound:.3e}")
        assert gap <= bound
    b = R.cached("b", name)      # and the contract itself, bit for bit: one slice, ascending index
    assert got["shifted"].tobytes() == b["shifted"].tobytes() and got["iterations"] == b["iterations"] and got["modes"].shape == b["modes"].shape


def test_more_than_one_slice_follows_the_stated_order(cl):
    """unquantised points, two slices, an RBF kernel: the f64 sums are not exact, and the result is the contract's slice-by-slice sum bit for bit"""
    p = R.unit_blobs_nd(6, per=400)
    seeds = np.ascontiguousarray(p[::40])
    prm = dict(kernel_radius=2.0, max_iter=3, cluster_tol=0.2, convergence_tol=1e-7)
    for kind, sigma in ((R.UNITY, 1.0), (R.RBF, 0.8)):
        want = R.contract_nd(p, seeds, kind=kind, sigma=sigma, **prm)
        assert set(want["slices"]) == {2}
        got = run(cl, p, seeds, kind=kind, sigma=sigma, **prm)
        assert got["stats"]["slices_first"] == 2 and got["shifted"].tobytes() == want["shifted"].tobytes() and got["iterations"] == want["iterations"] == 3


# ---- repeat run ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(cl):
    p = R.unit_blobs_nd(9, per=400)      # two slices
    for kind, sigma in ((R.UNITY, 1.0), (R.RBF, 0.8)):
        a = run(cl, p, None, kind=kind, sigma=sigma, **R.UNIT)
        b = run(cl, p, None, kind=kind, sigma=sigma, **R.UNIT)
        assert a["iterations"] == b["iterations"] > 3 and a["stats"]["slices_first"] == 2
        for k in EXACT + ("modes",):
            assert a[k].tobytes() == b[k].tobytes(), (kind, k)


# ---- mirrors -------------------------------------------------------------------------------------------------------------------------------
def test_python_classes(cl):
    import cilantro_amd

    for dim, cls in ((2, cilantro_amd.MeanShift2f), (6, cilantro_amd.MeanShiftXf)):
        _, p, _, prm = R.fixture(f"lattice_{dim}")
        want = R.cached("b", f"lattice_{dim}")
        ms = cls(p).cluster(prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"], cl.UnityWeightEvaluator())
        assert ms.getNumberOfClusters() == 3 and ms.getNumberOfPerformedIterations() == want["iterations"] and ms.dim == dim
        assert np.array_equal(ms.getShiftedSeeds(), want["shifted"]) and np.array_equal(ms.getPointToClusterIndexMap(), want["labels"]) and ms.getClusterModes().shape == (3, dim)
        segs = ms.getClusterToPointIndicesMap()
        assert all(np.array_equal(sg, want["members"][want["offsets"][c]:want["offsets"][c + 1]]) for c, sg in enumerate(segs))
        seeds = R.lattice_seeds_nd(dim)
        want = R.cached("b", f"lattice_seeds_{dim}")
        ms.cluster(seeds, prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"])
        assert ms.getNumberOfClusters() == 3 and np.array_equal(ms.getShiftedSeeds(), want["shifted"]) and np.array_equal(ms.getPointToClusterIndexMap(), want["labels"])
        assert np.diff(want["offsets"]).tolist() == [len(sg) for sg in ms.getClusterToPointIndicesMap()]


def test_cpp_mirrors_give_the_python_mirror_results(cl, tmp_path):
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_mean_shift_nd.cpp"), "test_mean_shift_nd")
    for dim in (2, 9):
        p, seeds = R.unit_blobs_nd(dim), R.unit_blobs_nd(dim, per=20, seed=1)
        fp, fs = str(tmp_path / f"p{dim}.f32"), str(tmp_path / f"s{dim}.f32")
        p.tofile(fp)
        seeds.tofile(fs)
        for tag, sd, sarg, kind, sigma in (("all", None, "-", 0, 1.0), ("own", seeds, fs, 2, 0.8)):
            pre = str(tmp_path / f"{tag}{dim}")
            r = subprocess.run([exe, "run", str(dim), fp, sarg, pre, "2", "5000", "0.2", "1e-7", str(kind), str(sigma)], capture_output=True, text=True)
            assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
            want = run(cl, p, sd, np.float32(2.0), 5000, np.float32(0.2), np.float32(1e-7), kind=kind, sigma=np.float32(sigma))
            u64 = lambda v: np.fromfile(f"{pre}.{v}.u64", np.uint64).astype(np.int64)      # noqa: E731
            f32 = lambda v: np.fromfile(f"{pre}.{v}.f32", np.float32).reshape(-1, dim)      # noqa: E731
            assert u64("iters")[0] == want["iterations"] > 3 and np.array_equal(u64("labels"), want["labels"]) and np.array_equal(u64("members"), want["members"])
            assert np.array_equal(u64("sizes"), np.diff(want["offsets"])) and f32("shifted").tobytes() == want["shifted"].tobytes() and f32("modes").tobytes() == want["modes"].tobytes()


def test_example_output():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(os.path.dirname(HERE), "examples", "mean_shift_nd.cpp"), "example_mean_shift_nd")
    outs = []
    for _ in range(2):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if not ln.startswith("Clustering time")])
    assert outs[0] == outs[1]      # the same bits twice
    text = "\n".join(outs[0])
    assert "Number of points: 1500 (dimension 6)" in text
    k = int(re.search(r"Number of clusters: (\d+)", text).group(1))
    it = int(re.search(r"Performed mean shift iterations: (\d+)", text).group(1))
    lo, hi = (int(g) for g in re.search(r"Cluster size range is: \[(\d+),(\d+)\]", text).groups())
    modes = re.findall(r"mode \d+: \(([^)]*)\), (\d+) seeds", text)
    assert 1 <= k <= 1500 and 1 <= it <= 5000 and 1 <= lo <= hi <= 1500 and len(modes) == min(k, 10)
    assert all(len(m[0].split(",")) == 6 for m in modes) and max(int(m[1]) for m in modes) <= hi and (k > 10 or sum(int(m[1]) for m in modes) == 1500)
