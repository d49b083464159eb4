"""CPU: the yardstick of the robust (MCD) normal estimation (tests/_robust_normal_refs.py, the numpy restatement of DESIGN.md section 15.1)
-- its sampler against csrc/ransac_sampling.hpp, its h table, and what the contract buys on a plane with planted off-surface points --, the
argument rules of the C entry (they hold without a device), and the g++ build of the C++ mirror and the example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _normal_refs as nr
import _robust_normal_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_sampler_equals_draw_samples():
    """every elemental start the kernel can draw for the printed (seed, row, trial, m): seeds at both ends of 64 bits, m = 4..32, rows up to 2^32 - 17"""
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_mcd_sampling.cpp"), "test_mcd_sampling")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 5 * 8 * 4 * 29
    rows, ms = set(), set()
    for line in lines:
        seed, row, trial, m, p0, p1, p2 = (int(v) for v in line.split())
        pick = R.draw3(R.trial_seed(seed, row, trial), m)
        assert pick == [p0, p1, p2], line
        assert len(set(pick)) == 3 and max(pick) < m
        rows.add(row)
        ms.add(m)
    assert max(rows) == (1 << 32) - 17 and ms == set(range(4, 33))


def test_h_table():
    """h = min(max(3, llroundf(ratio * m)), m): 0.75 m and 0.5 m are exact in f32, so the table is integer arithmetic -- halves round away from zero"""
    for m in range(3, 33):
        assert R.h_of(0.75, m) == min(max(3, (3 * m + 2) // 4), m)
        assert R.h_of(0.5, m) == min(max(3, (m + 1) // 2), m)
        assert R.h_of(1.0, m) == m
    assert [R.h_of(0.75, m) for m in (3, 4, 5, 6, 10, 12, 32)] == [3, 3, 4, 5, 8, 9, 24]      # 4.5 -> 5, 7.5 -> 8
    assert [R.h_of(0.5, m) for m in (4, 5, 7, 12, 31, 32)] == [3, 3, 4, 6, 16, 16]             # 2.5 -> 3, 3.5 -> 4, 15.5 -> 16
    assert R.h_of(3e38, 32) == 32 and R.h_of(1e-30, 32) == 3


@pytest.fixture(scope="module")
def planted(orc):
    x, out = R.planted_cloud()
    idx, cnt, _ = nr.oracle_lists(orc, x, ("knn", 12, np.inf))
    return x, out, idx, cnt


def test_planted_outliers_tilt_and_flags(planted):
    """a jittered plane, 10 % of its points planted 0.5 .. 1.5 lattice steps off it, k = 12, (T, R) = (6, 3).  Over the rows whose list holds
    1..3 planted points: the median tilt of the robust normal from +z is below a tenth of plain PCA's; with chi = 6.25 at least 90 % of
    the planted points are flagged and at most 15 % of the clean ones."""
    x, out, idx, cnt = planted
    assert (cnt == 12).all() and 80 < out.sum() < 130
    held = out[idx].sum(axis=1)
    rows = (held >= 1) & (held <= 3)
    assert rows.sum() > 400
    for seed in (0, 11):
        rob = R.robust(x, idx, cnt, 6, 3, 0.75, -1.0, seed)
        assert rob.won.all() and rob.inlier.all() and (rob.sel.sum(axis=1) == 9).all()
        plain = R.robust(x, idx, cnt, 6, 3, 1.0, -1.0, seed)
        assert not plain.ran.any() and (plain.mask == 0xFFF).all()
        t_rob = np.median(R.tilt_degrees(R.normals_of(rob.C))[rows])
        t_plain = np.median(R.tilt_degrees(R.normals_of(plain.C))[rows])
        chi = R.robust(x, idx, cnt, 6, 3, 0.75, 6.25, seed)
        assert np.array_equal(chi.mask, rob.mask)      # the threshold labels, it does not choose
        flagged = chi.inlier == 0
        hit, false = flagged[rows & out].mean(), flagged[rows & ~out].mean()
        print(f"seed {seed}: rows {int(rows.sum())}, median tilt robust {t_rob:.3f} deg, plain {t_plain:.3f} deg; planted flagged {hit:.3f} ({int((rows & out).sum())}), "
              f"clean flagged {false:.3f} ({int((rows & ~out).sum())})")
        assert t_rob < 0.1 * t_plain
        assert hit >= 0.90 and false <= 0.15


def test_another_seed_changes_some_subsets_and_none_without_trials(planted):
    """(the seed meets the row and the trial by xor: seeds that differ only below bit 6 hand the same starts to other trials of the row)"""
    x, out, idx, cnt = planted
    a, b = R.robust(x, idx, cnt, 2, 1, 0.75, 6.25, 0), R.robust(x, idx, cnt, 2, 1, 0.75, 6.25, 20240607)
    assert (a.mask != b.mask).any()
    swapped = R.robust(x, idx, cnt, 2, 1, 0.75, 6.25, 1)      # seed 1: trial 0 and trial 1 of seed 0, exchanged
    assert (swapped.mask != a.mask).mean() < 0.01
    a, b = R.robust(x, idx, cnt, 2, 1, 1.0, 6.25, 0), R.robust(x, idx, cnt, 2, 1, 1.0, 6.25, 20240607)
    assert np.array_equal(a.mask, b.mask) and np.array_equal(a.inlier, b.inlier)


# ---- argument rules: before any device is opened ------------------------------------------------------------------------------
def call(L, n=4, points=True, params=True, normals=True, mem=0, **fields):
    from cilantro_amd import capi

    pts = np.zeros((4, 3), np.float32)
    prm = capi.McdParams()
    L.cilhip_mcd_params_default(C.byref(prm))
    prm.k = 3
    for key, v in fields.items():
        setattr(prm, key, v)
    nrm, cur = np.full(12, 7, np.float32), np.full(4, 7, np.float32)
    mask, inl = np.full(4, 7, np.uint32), np.full(4, 7, np.uint8)
    rc = L.cilhip_robust_normals_knn3f(0, pts.ctypes.data if points else None, n, mem, C.byref(prm) if params else None, None, nrm.ctypes.data if normals else None,
                                       cur.ctypes.data, mask.ctypes.data, inl.ctypes.data)
    untouched = all((a == 7).all() for a in (nrm, cur, mask, inl))
    return rc, untouched, L.cilhip_last_error(None).decode()


def test_refused_input_needs_no_device(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    prm = capi.McdParams()
    L.cilhip_mcd_params_default(C.byref(prm))
    assert (prm.num_trials, prm.num_refinements, prm.k, prm.seed) == (6, 3, 0, 0) and prm.inlier_ratio == 0.75 and prm.chi_square_threshold == -1.0 and np.isinf(prm.max_sq_dist)
    nan, inf = float("nan"), float("inf")
    for kw, word in (({"params": False}, "params is null"), ({"points": False}, "xyz is null"), ({"normals": False}, "normals_out is null"), ({"k": 0}, "k must be"), ({"k": 33}, "k must be"),
                     ({"num_trials": 0}, "num_trials"), ({"num_trials": 65}, "num_trials"), ({"num_refinements": -1}, "num_refinements"), ({"num_refinements": 17}, "num_refinements"),
                     ({"inlier_ratio": nan}, "inlier_ratio"), ({"inlier_ratio": inf}, "inlier_ratio"), ({"inlier_ratio": 0.0}, "inlier_ratio"), ({"inlier_ratio": -0.5}, "inlier_ratio"),
                     ({"chi_square_threshold": nan}, "chi_square_threshold"), ({"n": (1 << 32) - 16}, "n must be below"), ({"n": 1 << 33}, "n must be below"), ({"mem": 2}, "mem"),
                     ({"mem": -1}, "mem")):
        rc, untouched, err = call(L, **kw)
        assert rc == capi.ERR_INVALID and untouched and word in err and err.startswith("robust_normals: "), (kw, rc, err)
    import torch

    if not torch.cuda.is_available():      # a valid call fails loudly: there is no CPU path
        for kw in ({}, {"chi_square_threshold": inf}, {"chi_square_threshold": -inf}, {"num_trials": 64, "num_refinements": 16, "k": 32}):
            rc, untouched, err = call(L, **kw)
            assert rc == capi.ERR_NO_DEVICE and untouched and "no CPU path" in err, (kw, rc, err)
        from cilantro_amd.normal_estimation import RobustNormalEstimation3f

        with pytest.raises(capi.CilhipError):
            RobustNormalEstimation3f(np.zeros((4, 3), np.float32)).getNormalsKNN(3)


def test_python_class_settings_and_radius_refusals(hip_lib):
    from cilantro_amd.normal_estimation import RobustNormalEstimation3f

    ne = RobustNormalEstimation3f(np.zeros((4, 3), np.float32))
    m = ne.covarianceMethod()
    assert (m.getNumberOfTrials(), m.getNumberOfRefinements(), m.getInlierRatio(), m.getChiSquareThreshold(), m.getSeed()) == (6, 3, 0.75, -1.0, 0)
    assert m.setChiSquareThreshold(6.25).setNumberOfTrials(2).setNumberOfRefinements(1).setInlierRatio(0.5).setSeed(9) is m
    assert (m.getNumberOfTrials(), m.getNumberOfRefinements(), m.getInlierRatio(), m.getChiSquareThreshold(), m.getSeed()) == (2, 1, 0.5, 6.25, 9)
    assert np.isnan(ne.getViewPoint()).all() and ne.setViewPoint([0, 0, 0]) is ne and (ne.getViewPoint() == 0).all()
    for getter in (ne.getNormalsRadius, ne.getCurvatureRadius, ne.getNormalsAndCurvatureRadius):
        with pytest.raises(ValueError, match="KNNInRadius"):
            getter(0.1)


# ---- the C++ mirror and the example compile with g++ ----------------------------------------------------------------------------
def test_cpp_mirror_and_example_compile():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_robust_normals.cpp"), "test_robust_normals")
    build_cpp(os.path.join(ROOT, "examples", "robust_normal_estimation.cpp"), "example_robust_normal_estimation")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "robust_normal_estimation.cpp")).read()
    for needle in ("cloud.gridDownsample(0.005f)", "setChiSquareThreshold(6.25f).setNumberOfTrials(2).setNumberOfRefinements(1)", "ne.getNormalsKNN(12)", "removeInvalidNormals()",
                   "setViewPoint(0.0f, 0.0f, 0.0f)"):
        assert needle in src, needle
