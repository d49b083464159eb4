"""GPU: mean-shift clustering (cilhip_mean_shift3f and its Python / C++ mirrors) against the numpy yardsticks of tests/_meanshift_refs.py
(pinned on the CPU by tests/test_meanshift_refs_cpu.py, which also asserts the margins these fixtures need).  On the 2^-10 lattice with
the flat kernel every f64 sum is exact in any order, so the whole trajectory is compared with np.array_equal; elsewhere the bounds are
the derived ones of DESIGN.md section 13."""
import os
import subprocess

import numpy as np
import pytest

import _meanshift_refs as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXACT = ("shifted", "labels", "offsets", "members")


@pytest.fixture(scope="module")
def cl():
    from cilantro_amd import clustering

    return clustering


def evaluator(cl, kind, sigma=1.0):
    return (cl.UnityWeightEvaluator(), cl.IdentityWeightEvaluator(), cl.RBFKernelWeightEvaluator(sigma))[kind]


def run(cl, points, seeds, kernel_radius, max_iter, cluster_tol, convergence_tol=np.finfo(np.float32).eps, kind=0, sigma=1.0, form=0, device_mem=False):
    """one call -> the result with every array as numpy"""
    if device_mem:
        import torch

        points = torch.from_numpy(np.ascontiguousarray(points, np.float32)).cuda()
        seeds = None if seeds is None else torch.from_numpy(np.ascontiguousarray(seeds, np.float32)).cuda()
    r = cl.mean_shift(points, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator(cl, kind, sigma), seeds=seeds, form=form)
    if device_mem:
        assert all(r[k].is_cuda for k in EXACT + ("modes",))
        r = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    return r


def same(got, want, what=EXACT):
    for k in what:
        assert np.array_equal(got[k], want[k], equal_nan=(k in ("shifted", "modes"))), k
    assert got["iterations"] == want["iterations"], (got["iterations"], want["iterations"])


# ---- exact trajectory ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("own_seeds", [False, True])
def test_exact_trajectory_on_the_lattice(cl, own_seeds):
    name = "lattice_seeds" if own_seeds else "lattice"
    _, p, s, prm = next(f for f in R.margin_fixtures() if f[0] == name)
    want = R.cached("b", name)
    assert want["iterations"] == 6 and len(want["leaders"]) == 3
    for form in (1, 2, 0):
        for device_mem in (False, True):
            got = run(cl, p, s, form=form, device_mem=device_mem, **prm)
            same(got, want)
            assert got["stats"]["form_used"] == (form or got["stats"]["form_used"]) and got["stats"]["form_used"] in (1, 2)
            assert got["stats"]["passes"] == 6 and got["stats"]["rounds"] >= 1
            assert np.array_equal(got["members"][got["offsets"][:-1]], want["leaders"])      # a cluster's first member is its leader


# ---- single step: derived bound against the exact rational mean ----------------------------------------------------------------
@pytest.mark.parametrize("kind,sigma", [(R.IDENTITY, 1.0), (R.RBF, 0.15)])
def test_single_step_is_within_the_derived_bound(cl, kind, sigma):
    p = R.offset_cloud()
    seeds = np.ascontiguousarray(p[::5] + np.float32(0.01))
    radius = np.float32(0.4)
    r2 = radius * radius
    exact = [R.exact_step(s, p, r2, kind, sigma) for s in seeds]
    m, bound = np.array([e[0] for e in exact]), np.array([e[1] for e in exact])
    assert max(e[2] for e in exact) > 20
    for form in (1, 2):
        got = run(cl, p, seeds, radius, 1, 0.05, kind=kind, sigma=sigma, form=form)
        err = np.abs(got["shifted"].astype(np.float64) - m)
        print(f"kind {kind} form {form}: max err / bound = {(err / bound).max():.3f}, largest error {err.max():.3e}")
        assert got["iterations"] == 1 and (err <= bound).all()


# ---- grouping alone (max_iter = 0): exact against the serial first-fit ---------------------------------------------------------------
def grouping_check(cl, seeds, tol):
    labels, leaders = R.first_fit(seeds, tol)
    offsets, members = R.lists_of(labels, len(leaders))
    got = run(cl, np.zeros((3, 3), np.float32), seeds, 1.0, 0, tol)
    assert got["iterations"] == 0 and np.array_equal(got["shifted"], seeds, equal_nan=True)
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["offsets"], offsets) and np.array_equal(got["members"], members)
    assert np.array_equal(got["members"][got["offsets"][:-1]], leaders)
    return got, leaders


def test_grouping_equals_the_serial_first_fit(cl):
    from test_meanshift_refs_cpu import grouping_cases

    for name, seeds, tol in grouping_cases():
        got, leaders = grouping_check(cl, seeds, tol)
        if name == "chain":      # about one round per leader, and it finishes
            assert len(leaders) == 100 and got["stats"]["rounds"] == 100
        if name == "collapsed":
            assert len(leaders) == 3 and got["stats"]["rounds"] == 1 and sorted(np.diff(got["offsets"]).tolist())[0] > 600
        if name == "duplicates_tol0":
            assert len(leaders) == seeds.shape[0]
        if name == "one_mode":
            # the seeds' grid keeps its cells at the tolerance: refined to the seeds' spread, one ball was 10^7 cells and this took 7.3 s
            assert len(leaders) == 1 and got["stats"]["rounds"] == 1 and got["stats"]["group_ms"] < 500.0


# ---- modes ------------------------------------------------------------------------------------------------------------------------------
def test_modes_are_within_the_derived_bound_of_the_exact_member_mean(cl):
    _, p, s, prm = next(f for f in R.margin_fixtures() if f[0] == "unit")
    runs = [run(cl, p, s, **prm), run(cl, np.zeros((3, 3), np.float32), R.collapsed_seeds(), 1.0, 0, 0.01)]
    for got in runs:
        k = len(got["offsets"]) - 1
        assert got["modes"].shape == (k, 3) and k >= 2
        for c in range(k):
            m, bound = R.exact_mode(got["shifted"], got["members"][got["offsets"][c]:got["offsets"][c + 1]])
            assert (np.abs(got["modes"][c].astype(np.float64) - m) <= bound).all(), c


# ---- edge rules -------------------------------------------------------------------------------------------------------------------------
def test_empty_ball_becomes_a_nan_singleton_and_the_count_is_max_iter(cl):
    p = R.lattice_blobs()
    seeds = np.concatenate([R.lattice_seeds()[:10], R.quantise([[7.5, 7.5, 7.5]]), R.lattice_seeds()[10:20]])
    prm = dict(R.LATTICE, max_iter=40)
    want = R.contract(p, seeds, **prm)
    assert want["iterations"] == 40 and np.isnan(want["shifted"][10]).all() and np.isfinite(np.delete(want["shifted"], 10, axis=0)).all()
    for form in (1, 2):
        got = run(cl, p, seeds, form=form, **prm)
        same(got, want)
        c = got["labels"][10]
        assert got["stats"]["passes"] < 40 and np.diff(got["offsets"])[c] == 1 and np.isnan(got["modes"][c]).all() and np.isfinite(np.delete(got["modes"], c, axis=0)).all()


def test_non_finite_seeds_and_points(cl):
    p = R.lattice_blobs()
    seeds = R.lattice_seeds().copy()
    seeds[3, 1], seeds[17, 0], seeds[40] = np.nan, np.inf, -np.inf
    want = R.contract(p, seeds, **R.LATTICE)
    assert want["iterations"] == R.LATTICE["max_iter"] and np.isnan(want["shifted"][[3, 17, 40]]).all()
    for form in (1, 2):
        same(run(cl, p, seeds, form=form, **R.LATTICE), want)
    # NaN / inf data points are in no ball: the others see the cloud without those rows
    rng = np.random.default_rng(9)
    bad = rng.permutation(p.shape[0])[:30]
    q = p.copy()
    q[bad[:10], 0], q[bad[10:20], 2], q[bad[20:], 1] = np.nan, np.inf, -np.inf
    q[-1] = np.nan
    clean = q[np.isfinite(q).all(axis=1)]
    good_seeds = R.lattice_seeds()
    want = R.contract(clean, good_seeds, **R.LATTICE)
    for form in (1, 2):
        for device_mem in (False, True):
            same(run(cl, q, good_seeds, form=form, device_mem=device_mem, **R.LATTICE), want)
    # ... and with every point a seed, the non-finite rows are NaN singletons and the rest is what the clean cloud's seeds do
    got = run(cl, q, None, **R.LATTICE)
    ok = np.isfinite(q).all(axis=1)
    ref = R.contract(clean, None, **dict(R.LATTICE, max_iter=got["iterations"]))
    assert got["iterations"] == R.LATTICE["max_iter"] and np.array_equal(got["shifted"][ok], ref["shifted"]) and np.isnan(got["shifted"][~ok]).all()
    assert len(got["offsets"]) - 1 == len(ref["leaders"]) + int((~ok).sum())


def test_no_points_with_seeds(cl):
    seeds = R.lattice_seeds()[:9]
    for form in (1, 2, 0):
        got = run(cl, np.zeros((0, 3), np.float32), seeds, 1.0, 7, 0.25, form=form)
        assert got["iterations"] == 7 and np.isnan(got["shifted"]).all() and np.array_equal(got["labels"], np.arange(9))
        assert np.array_equal(got["offsets"], np.arange(10)) and np.array_equal(got["members"], np.arange(9)) and np.isnan(got["modes"]).all()
    got = run(cl, np.zeros((0, 3), np.float32), seeds, 1.0, 0, 0.25)      # no pass: the seeds as they came, grouped
    assert got["iterations"] == 0 and np.array_equal(got["shifted"], seeds)


def test_rbf_weights_below_the_cut_give_the_nan_rule(cl):
    from oracle import oracle as orc

    p = R.lattice_blobs()
    seeds = (R.lattice_seeds()[:12] + np.float32(2.0 ** -11)).astype(np.float32)      # half a lattice step off every point
    sigma = 1e-5
    d2 = R.d2_pinned(seeds, p)
    inside = d2 < np.float32(1.0)
    assert inside.any(axis=1).all() and (R.rbf_coeff(sigma) * d2[inside] < -80).all() and not orc.pinned_expf(R.rbf_coeff(sigma) * d2[inside]).any()
    for form in (1, 2):
        got = run(cl, p, seeds, 1.0, 5, 0.25, kind=R.RBF, sigma=sigma, form=form)
        assert got["iterations"] == 5 and got["stats"]["passes"] == 1 and np.isnan(got["shifted"]).all() and np.array_equal(got["labels"], np.arange(12))


def test_one_pass_leaves_unconverged_seeds_grouped_as_they_stand(cl):
    p = R.lattice_blobs()
    prm = dict(R.LATTICE, max_iter=1)
    want = R.contract(p, None, **prm)
    assert want["iterations"] == 1 and len(want["leaders"]) > 3      # not converged: more clusters than modes
    for form in (1, 2):
        same(run(cl, p, None, form=form, **prm), want)


# ---- end to end against the literal transcription ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [f[0] for f in R.margin_fixtures()])
def test_end_to_end_against_the_literal_transcription(cl, name):
    _, p, s, prm = next(f for f in R.margin_fixtures() if f[0] == name)
    a = R.cached("a", name)
    # four times the largest (a)-vs-(b) gap the CPU test measured (R.RECORDED_GAP = 2.9e-6, on unit-scale blobs): the factor covers a
    # fixture of another scale
    bound = 4.0 * R.RECORDED_GAP
    for form in (1, 2, 0):
        got = run(cl, p, s, form=form, **prm)
        assert np.array_equal(got["labels"], a["labels"]) and len(got["offsets"]) - 1 == len(a["leaders"])
        gap = float(np.abs(got["shifted"].astype(np.float64) - a["shifted"].astype(np.float64)).max())
        print(f"{name} form {form}: passes {got['iterations']} (literal {a['iterations']}), max |shifted - literal| = {gap:.3e}, bound {bound:.3e}")
        assert gap <= bound


# ---- repeat run ----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical(cl):
    p = R.unit_blobs()
    for form in (1, 2):
        for kind, sigma in ((R.UNITY, 1.0), (R.RBF, 0.8)):
            a = run(cl, p, None, kind=kind, sigma=sigma, form=form, **R.UNIT)
            b = run(cl, p, None, kind=kind, sigma=sigma, form=form, **R.UNIT)
            assert a["iterations"] == b["iterations"] > 3
            for k in EXACT + ("modes",):
                assert a[k].tobytes() == b[k].tobytes(), (form, kind, k)


# ---- mirrors -------------------------------------------------------------------------------------------------------------------------------
def test_python_class(cl):
    _, p, _, prm = next(f for f in R.margin_fixtures() if f[0] == "lattice")
    want = R.cached("b", "lattice")
    ms = cl.MeanShift3f(p).cluster(prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"], cl.UnityWeightEvaluator())
    assert ms.getNumberOfClusters() == 3 and ms.getNumberOfPerformedIterations() == 6
    assert np.array_equal(ms.getShiftedSeeds(), want["shifted"]) and np.array_equal(ms.getPointToClusterIndexMap(), want["labels"]) and ms.getClusterModes().shape == (3, 3)
    segs = ms.getClusterToPointIndicesMap()
    assert all(np.array_equal(sg, want["members"][want["offsets"][c]:want["offsets"][c + 1]]) for c, sg in enumerate(segs))
    seeds = R.lattice_seeds()
    want = R.cached("b", "lattice_seeds")
    ms.cluster(seeds, prm["kernel_radius"], prm["max_iter"], prm["cluster_tol"], prm["convergence_tol"])
    assert ms.getNumberOfClusters() == 3 and np.array_equal(ms.getShiftedSeeds(), want["shifted"]) and np.array_equal(ms.getPointToClusterIndexMap(), want["labels"])
    assert np.diff(want["offsets"]).tolist() == [len(sg) for sg in ms.getClusterToPointIndicesMap()]


def test_cpp_mirror_gives_the_python_mirror_results(cl, tmp_path):
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_mean_shift.cpp"), "test_mean_shift")
    p, seeds = R.unit_blobs(), R.unit_blobs(per=20, seed=1)
    fp, fs = str(tmp_path / "p.f32"), str(tmp_path / "s.f32")
    p.tofile(fp)
    seeds.tofile(fs)
    for tag, sd, sarg, kind, sigma in (("all", None, "-", 0, 1.0), ("own", seeds, fs, 2, 0.8)):
        pre = str(tmp_path / tag)
        r = subprocess.run([exe, "run", fp, sarg, pre, "2", "5000", "0.2", "1e-7", str(kind), str(sigma)], capture_output=True, text=True)
        assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
        want = run(cl, p, sd, np.float32(2.0), 5000, np.float32(0.2), np.float32(1e-7), kind=kind, sigma=np.float32(sigma))
        u64 = lambda v: np.fromfile(f"{pre}.{v}.u64", np.uint64).astype(np.int64)      # noqa: E731
        f32 = lambda v: np.fromfile(f"{pre}.{v}.f32", np.float32).reshape(-1, 3)      # noqa: E731
        assert u64("iters")[0] == want["iterations"] > 3 and np.array_equal(u64("labels"), want["labels"]) and np.array_equal(u64("members"), want["members"])
        assert np.array_equal(u64("sizes"), np.diff(want["offsets"])) and f32("shifted").tobytes() == want["shifted"].tobytes() and f32("modes").tobytes() == want["modes"].tobytes()
