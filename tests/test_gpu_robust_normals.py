"""GPU: robust (MCD) normal estimation -- cilhip_robust_normals_knn3f and its Python / C++ mirrors -- against the numpy restatement of
the contract (tests/_robust_normal_refs.py; pinned on the CPU by tests/test_robust_normal_refs_cpu.py).

The decisions -- the final subset of every row and its inlier flag -- are compared for equality, every row, none left out: the kernel and
the restatement perform the same IEEE operations in the same order, so there is nothing to tolerate.  The normals and curvatures are
checked like the plain estimator's: inside the a-priori bounds of tests/_normal_refs.py around the f64 PCA of the row's selected subset.
The neighbour lists the restatement works on come from the CPU oracle, never from the product."""
import os
import subprocess

import numpy as np
import pytest

import _normal_refs as nr
import _robust_normal_refs as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SETTINGS = tuple((t, r, ratio) for (t, r) in ((1, 0), (2, 1), (6, 3)) for ratio in (0.75, 0.5))
EDGE_KS = (4, 12, 32)
SEED = 0x5EED0123456789


@pytest.fixture(scope="module")
def p1():
    return nr.frame()


def estimator(x, trials, refinements, ratio, chi, seed=SEED, vp=None):
    from cilantro_amd.normal_estimation import RobustNormalEstimation3f

    ne = RobustNormalEstimation3f(x).setViewPoint(vp)
    ne.covarianceMethod().setNumberOfTrials(trials).setNumberOfRefinements(refinements).setInlierRatio(ratio).setChiSquareThreshold(chi).setSeed(seed)
    return ne


def run(x, k, r2, trials, refinements, ratio, chi, seed=SEED, vp=None):
    """one call with a SQUARED radius passed as it is -> (normals, curvature, masks, inliers) as numpy"""
    out = estimator(x, trials, refinements, ratio, chi, seed, vp)._run(k, float(r2), True, True)
    return tuple(o.cpu().numpy() if hasattr(o, "cpu") else o for o in out)


_lists = {}


def lists(orc, tag, x, k, r2):
    key = (tag, k, float(r2))
    if key not in _lists:
        idx, cnt, _ = nr.oracle_lists(orc, x, ("knn", k, r2))
        _lists[key] = (idx, cnt)
    return _lists[key]


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def decisions_equal(orc, tag, x, k, r2, chi=6.25, settings=SETTINGS):
    """masks and inlier flags of every row against the restatement, for every (T, R, ratio) -> {setting: rows that ran trials}"""
    idx, cnt = lists(orc, tag, x, k, r2)
    ran = {}
    for trials, refinements, ratio in settings:
        want = R.robust(x, idx, cnt, trials, refinements, ratio, chi, SEED)
        _, _, mask, inl = run(x, k, r2, trials, refinements, ratio, chi)
        bad = np.nonzero((mask.view(np.uint32) != want.mask) | (inl != want.inlier))[0]
        assert len(bad) == 0, (tag, k, float(r2), trials, refinements, ratio, len(bad), bad[:5].tolist(), [hex(int(v)) for v in mask[bad[:5]]], [hex(int(v)) for v in want.mask[bad[:5]]],
                               inl[bad[:5]].tolist(), want.inlier[bad[:5]].tolist())
        ran[(trials, refinements, ratio)] = int(want.ran.sum())
    return ran, cnt


# ---- 1. exact decisions --------------------------------------------------------------------------------------------------------------
def named_clouds(p1):
    return {"planted": (R.planted_cloud()[0], 12), "frame 5000": (nr.edge_cloud(p1, 5000), 12), "plane lattice": (nr.plane_lattice(), 9), "line": (nr.line_cloud(), 5),
            "repeated points": (nr.repeated_points(), 8), "doubled frame": (nr.doubled_frame(p1), 12)}


@pytest.mark.parametrize("name", ("planted", "frame 5000", "plane lattice", "line", "repeated points", "doubled frame"))
def test_decisions_equal_the_restatement(orc, hip_lib, p1, name):
    """the planted plane; 5 000 points of the raw sensor frame (depth quantisation makes many 9-subsets coplanar: det <= 0, rounding
    decides -- deliberately included); an exact plane, a line, two repeated points and doubled points (zero and singular covariances)"""
    x, k = named_clouds(p1)[name]
    ran, cnt = decisions_equal(orc, name, x, k, np.inf)
    print(name, "rows", len(x), "rows that ran trials per (T, R, ratio):", ran)
    assert all(v == len(x) for v in ran.values())      # k < n and no radius: every row ran its trials


@pytest.mark.parametrize("n", nr.EDGE_SIZES)
def test_decisions_equal_the_restatement_at_block_and_wave_edges(orc, hip_lib, p1, n):
    """n at the 64- and 256-lane edges and down to 3, k in (4, 12, 32) -- the three block sizes --, without a radius and inside one that
    leaves rows with m < k, m == 3 and m < 3"""
    x = nr.edge_cloud(p1, n)
    _, d2_3, cnt_3 = orc.knn_batch(orc.KDTree(x), x, 3, np.inf)
    r2 = np.float32(4.0) * nr.edge_radius_sq(d2_3, cnt_3)
    for k in EDGE_KS:
        ran, cnt = decisions_equal(orc, f"edge {n}", x, k, np.inf)
        assert (cnt == min(n, k)).all()
        ran_r, cnt_r = decisions_equal(orc, f"edge {n}", x, k, r2)
        print(f"n={n} k={k}: ran {ran}; in radius: m < 3: {int((cnt_r < 3).sum())}, m == 3: {int((cnt_r == 3).sum())}, 3 < m < k: {int(((cnt_r > 3) & (cnt_r < k)).sum())}, ran {ran_r}")
        if n >= 63 and k >= 12:
            assert (cnt_r < 3).any() and (cnt_r == 3).any() and ((cnt_r > 3) & (cnt_r < k)).any()


# ---- 2. normals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("planted", "frame 5000", "edge 257 in radius", "repeated points"))
def test_normals_are_the_pca_of_the_selected_subsets(orc, hip_lib, p1, name):
    """chi = -1: every normal and curvature inside the bounds of _normal_refs.check around the f64 PCA of the row's selected subset; the
    masks do not depend on chi; with chi = 6.25 the NaN rows are exactly the rows with m < 3 plus the rows with inlier == 0"""
    vp = np.float32([0.1, -0.2, 0.05])
    if name == "edge 257 in radius":
        x, k = nr.edge_cloud(p1, 257), 12
        _, d2_3, cnt_3 = orc.knn_batch(orc.KDTree(x), x, 3, np.inf)
        r2 = np.float32(4.0) * nr.edge_radius_sq(d2_3, cnt_3)
        tag = "edge 257"
    else:
        (x, k), r2, tag = named_clouds(p1)[name], np.inf, name
    idx, cnt = lists(orc, tag, x, k, r2)
    for trials, refinements, ratio in ((2, 1, 0.75), (6, 3, 0.5)):
        nrm, cur, mask, inl = run(x, k, r2, trials, refinements, ratio, -1.0, vp=vp)
        want = R.robust(x, idx, cnt, trials, refinements, ratio, -1.0, SEED)
        assert np.array_equal(mask, want.mask) and np.array_equal(inl, want.inlier) and np.array_equal(inl == 1, cnt >= 3)
        sub_idx, sub_cnt = R.subset_lists(idx, want.sel)
        res = nr.check(nr.reference(x, sub_idx, sub_cnt), nrm, cur, x, vp)
        print(name, (trials, refinements, ratio), {c: (r["rows"], r["violations"], r["worst ratio"]) for c, r in res.items()})
        assert not nr.violations(res), nr.violations(res)
        n6, c6, m6, i6 = run(x, k, r2, trials, refinements, ratio, 6.25, vp=vp)
        assert np.array_equal(m6, mask)
        nan_rows = np.isnan(n6).any(axis=1)
        assert np.array_equal(nan_rows, np.isnan(n6).all(axis=1)) and np.array_equal(nan_rows, i6 == 0) and np.array_equal(nan_rows, (cnt < 3) | (i6 == 0))
        assert np.isnan(c6[nan_rows]).all()
        keep = ~nan_rows
        assert n6[keep].tobytes() == nrm[keep].tobytes() and c6[keep].tobytes() == cur[keep].tobytes()      # the threshold labels, it does not choose
        if name in ("planted", "frame 5000"):
            assert 0 < (i6 == 0).sum() < len(x)


# ---- 3. plain equivalence --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (10, 32))
def test_ratio_one_is_the_plain_estimator_byte_for_byte(hip_lib, p1, k):
    from cilantro_amd.normal_estimation import NormalEstimation3f

    x = nr.edge_cloud(p1, 5000)
    for r2 in (np.inf, float(np.float32(0.02) * np.float32(0.02))):
        for vp in (None, np.zeros(3, np.float32)):
            nrm, cur, mask, inl = run(x, k, r2, 6, 3, 1.0, -1.0, vp=vp)
            pn, pc = NormalEstimation3f(x).setViewPoint(vp)._run(k, float(r2), True)
            assert same(nrm, pn) and same(cur, pc), (k, r2, vp)
            valid = ~np.isnan(pn).any(axis=1)
            assert np.array_equal(inl == 1, valid) and valid.sum() > 1000
            if np.isfinite(r2):
                assert (~valid).any() and (mask[valid] != 0).all() and (mask[~valid] == 0).all()
            else:
                assert (mask == (0xFFFFFFFF >> (32 - k))).all()


# ---- 4. repeat runs, memory spaces, seeds ------------------------------------------------------------------------------------------------
def test_runs_repeat_device_memory_equals_host_and_the_seed_matters(hip_lib):
    import torch

    x, _ = R.planted_cloud()
    a = run(x, 12, np.inf, 2, 1, 0.75, 6.25, vp=np.zeros(3, np.float32))
    b = run(x, 12, np.inf, 2, 1, 0.75, 6.25, vp=np.zeros(3, np.float32))
    assert all(same(u, v) for u, v in zip(a, b))
    xd = torch.from_numpy(x).cuda()
    d = estimator(xd, 2, 1, 0.75, 6.25, vp=np.zeros(3, np.float32))._run(12, np.inf, True, True)
    assert all(o.is_cuda for o in d)
    d = tuple(o.cpu().numpy() for o in d)
    assert same(d[0], a[0]) and same(d[1], a[1]) and same(d[2].view(np.uint32), a[2]) and same(d[3], a[3])
    other = run(x, 12, np.inf, 2, 1, 0.75, 6.25, seed=SEED + (1 << 20), vp=np.zeros(3, np.float32))
    assert (other[2] != a[2]).any()
    # h == m: no trials, nothing for a seed to change
    p = run(x, 12, np.inf, 2, 1, 1.0, 6.25, seed=1)
    q = run(x, 12, np.inf, 2, 1, 1.0, 6.25, seed=2)
    assert all(same(u, v) for u, v in zip(p, q))


# ---- 5. mirrors and the example --------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_gives_the_python_mirror_bytes(hip_lib, p1, tmp_path):
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_robust_normals.cpp"), "test_robust_normals")
    x = nr.edge_cloud(p1, 5000)
    fp = str(tmp_path / "p.f32")
    x.tofile(fp)
    for tag, radius, trials, refinements, ratio, chi, seed, vp in (("knn", 0.0, 2, 1, 0.75, 6.25, 77, 1), ("in_radius", 0.02, 6, 3, 0.5, -1.0, 5, 0)):
        pre = str(tmp_path / tag)
        r = subprocess.run([exe, "run", fp, pre, "12", repr(radius), str(trials), str(refinements), repr(ratio), repr(chi), str(seed), str(vp)], capture_output=True, text=True)
        assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
        ne = estimator(x, trials, refinements, ratio, chi, seed, np.zeros(3, np.float32) if vp else None)
        if radius:
            (nrm, cur), (mask, inl) = ne.getNormalsAndCurvatureKNNInRadius(12, radius), ne.getSubsetMasksAndInliersKNNInRadius(12, radius)
        else:
            (nrm, cur), (mask, inl) = ne.getNormalsAndCurvatureKNN(12), ne.getSubsetMasksAndInliersKNN(12)
        assert np.fromfile(pre + ".normals.f32", np.float32).tobytes() == nrm.tobytes() and np.fromfile(pre + ".curvature.f32", np.float32).tobytes() == cur.tobytes()
        assert np.array_equal(np.fromfile(pre + ".masks.u32", np.uint32), mask) and np.array_equal(np.fromfile(pre + ".inliers.u8", np.uint8), inl)
        assert same(ne.getNormalsKNN(12) if not radius else ne.getNormalsKNNInRadius(12, radius), nrm)
        assert 0 < np.isnan(nrm).any(axis=1).sum() < len(x) or chi < 0


def test_example_counts_the_invalid_normals_of_the_python_flow(hip_lib, p1, tmp_path):
    from test_components_refs_cpu import build_cpp

    from cilantro_amd.grid_downsampler import grid_downsample
    from cilantro_amd.ply_io import write_ply

    exe = build_cpp(os.path.join(os.path.dirname(HERE), "examples", "robust_normal_estimation.cpp"), "example_robust_normal_estimation")
    ply = str(tmp_path / "frame_1.ply")
    write_ply(ply, p1)
    r = subprocess.run([exe, ply], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {line.split(":")[0]: line.split(":")[1].strip() for line in r.stdout.strip().split("\n")}
    down = np.ascontiguousarray(grid_downsample(p1, 0.005)["points"], np.float32)
    nrm = estimator(down, 2, 1, 0.75, 6.25, 0, np.zeros(3, np.float32)).getNormalsKNN(12)
    invalid = int(np.isnan(nrm).any(axis=1).sum())
    print(r.stdout)
    assert int(got["Downsampled points"]) == len(down) and int(got["Invalid normals"]) == invalid and int(got["Valid normals"]) == len(down) - invalid
    assert 0 < invalid < len(down)
