"""Pins tests/_normal_refs.py (the f64 PCA reference and the per-row bounds the GPU normal tests check against) on the CPU.

`emulate` restates the product's documented arithmetic in numpy -- f64 sum of the neighbours rounded to an f32 mean, f32 differences
and f32 products (one rounding each), f64 sums, an f64 eigen-solve (eigh here, Jacobi there), the result rounded to f32, the view
point's dot product in f32 -- on the CPU oracle's neighbour lists.  It passes every check with zero violations on every input of
tests/test_gpu_normals.py: the bounds can be met by a correct implementation and are not tuned on the kernel.  Three injected
faults show that the checks bite."""
import numpy as np
import pytest

import _normal_refs as nr


def emulate(x, idx, cnt, view_point=None):
    """-> (normals f32 (n, 3), curvature f32 (n)) of self-queries with neighbour rows idx (padded with -1) / counts cnt"""
    x = np.asarray(x, np.float32).reshape(-1, 3)
    idx, cnt = np.asarray(idx, np.int64), np.asarray(cnt, np.int64)
    n, k = idx.shape
    nrm = np.full((n, 3), np.nan, np.float32)
    cur = np.full(n, np.nan, np.float32)
    for a in range(0, n, nr.CHUNK):
        rows = a + np.nonzero(cnt[a:a + nr.CHUNK] >= 3)[0]
        if not len(rows):
            continue
        live = np.arange(k)[None, :] < cnt[rows][:, None]
        m = cnt[rows].astype(np.float64)
        P = x[np.where(live, idx[rows], 0)]                                                        # f32 (r, k, 3)
        mean = (np.where(live[:, :, None], P.astype(np.float64), 0.0).sum(axis=1) / m[:, None]).astype(np.float32)
        t = P - mean[:, None, :]                                                                  # f32, one rounding
        assert t.dtype == np.float32
        C = np.empty((len(rows), 3, 3))
        for i in range(3):
            for j in range(i, 3):
                prod = t[:, :, i] * t[:, :, j]                                                    # f32, one rounding
                assert prod.dtype == np.float32
                C[:, i, j] = C[:, j, i] = np.where(live, prod.astype(np.float64), 0.0).sum(axis=1) / (m - 1.0)
        lam, vec = np.linalg.eigh(C)
        v = vec[:, :, 0].astype(np.float32)
        if view_point is not None:
            vp = np.asarray(view_point, np.float32).reshape(3)
            q = x[rows]
            d = v[:, 0] * (vp[0] - q[:, 0]) + (v[:, 1] * (vp[1] - q[:, 1]) + v[:, 2] * (vp[2] - q[:, 2]))
            assert d.dtype == np.float32
            v = np.where((d < 0)[:, None], -v, v)
        nrm[rows] = v
        with np.errstate(divide="ignore", invalid="ignore"):
            cur[rows] = (lam[:, 0] / ((lam[:, 2] + lam[:, 1]) + lam[:, 0])).astype(np.float32)
    return nrm, cur


def _covariance_error_ratio(x, idx, cnt, R):
    """largest ||C_emulated - C*||_F / Eb (the bound itself, before anything is derived from it)"""
    x = np.asarray(x, np.float32)
    worst = 0.0
    k = idx.shape[1]
    for a in range(0, len(idx), nr.CHUNK):
        rows = a + np.nonzero(cnt[a:a + nr.CHUNK] >= 3)[0]
        if not len(rows):
            continue
        live = np.arange(k)[None, :] < cnt[rows][:, None]
        m = cnt[rows].astype(np.float64)
        P = x[np.where(live, idx[rows], 0)]
        mean = (np.where(live[:, :, None], P.astype(np.float64), 0.0).sum(axis=1) / m[:, None]).astype(np.float32)
        t = P - mean[:, None, :]
        C = np.empty((len(rows), 3, 3))
        for i in range(3):
            for j in range(3):
                C[:, i, j] = np.where(live, (t[:, :, i] * t[:, :, j]).astype(np.float64), 0.0).sum(axis=1) / (m - 1.0)
        err = np.sqrt(((C - R.C[rows]) ** 2).sum(axis=(1, 2)))
        assert (R.Eb[rows] > 0).all()
        worst = max(worst, float((err / R.Eb[rows]).max()))
    return worst


@pytest.fixture(scope="module")
def p1():
    return nr.frame()


_lists = {}


def _case(orc, tag, x, call):
    key = (tag, call)
    if key not in _lists:
        idx, cnt, d2 = nr.oracle_lists(orc, x, call)
        _lists[key] = (idx, cnt, d2, nr.reference(x, idx, cnt))
    return _lists[key]


FRAME_TAGS = ("knn10", "knn32", "knn12_in_radius", "radius", "knn10_moved")


@pytest.mark.parametrize("tag", FRAME_TAGS)
def test_emulation_meets_every_bound_on_the_sensor_frame(orc, p1, tag):
    _, x, call, vp = next(c for c in nr.frame_cases(p1) if c[0] == tag)
    idx, cnt, d2, R = _case(orc, tag, x, call)
    nrm, cur = emulate(x, idx, cnt, vp)
    res = nr.check(R, nrm, cur, x, vp)
    cov = _covariance_error_ratio(x, idx, cnt, R)
    print(tag, "||E|| / Eb", cov, nr.summary(R, res, d2, cnt))
    assert not nr.violations(res), nr.violations(res)
    assert cov <= 1.0, cov
    assert res["rayleigh"]["rows"] == int((cnt >= 3).sum()) and res["nan pattern"]["rows"] == len(x)      # no row left out
    if tag == "knn10":
        assert nr.rows_with_equal_distances(d2, cnt).sum() * 3 > len(x)
    if tag == "radius":      # the k-NN-in-radius route lists what an exhaustive radius search lists
        sub = np.arange(0, len(x), 40)
        ci, cc = nr.padded_from_csr(*orc.radius_search(x, x[sub], call[1])[:2])
        assert cnt.max() == 46 and np.array_equal(cc, cnt[sub]) and np.array_equal(np.sort(ci, axis=1)[:, -46:], np.sort(idx[sub], axis=1)[:, -46:])
    if tag == "knn12_in_radius":
        assert (cnt < 3).sum() == 40 and (cnt < 12).sum() == 6067
    # sign free without a view point: the same normals negated row by row still pass, and fail the view-point check
    flip = nrm * np.where(np.arange(len(x)) % 2 == 0, np.float32(-1), np.float32(1))[:, None]
    assert not nr.violations(nr.check(R, flip, cur))
    assert nr.check(R, flip, cur, x, vp)["view point"]["violations"] > len(x) // 3


def test_emulation_meets_every_bound_on_the_small_and_degenerate_clouds(orc, p1):
    failures = []
    seen = 0
    cases = list(nr.edge_cases(orc, p1)) + list(nr.degenerate_cases(p1)) + list(nr.strict_cases())
    for name, x, call, vp in cases:
        idx, cnt, d2 = nr.oracle_lists(orc, x, call)
        R = nr.reference(x, idx, cnt)
        nrm, cur = emulate(x, idx, cnt, vp)
        res = nr.check(R, nrm, cur, x, vp)
        if nr.violations(res):
            failures.append((name, nr.violations(res)))
        if (cnt >= 3).any() and _covariance_error_ratio(x, idx, cnt, R) > 1.0:
            failures.append((name, "covariance error above Eb"))
        seen += 1
        # what the cases are there for
        if "radius" in name and name.startswith("n="):
            if not (cnt < 3).any():
                failures.append((name, "no row under 3 members"))
        if name.startswith("n=3/knn") and "radius" not in name:
            if not ((cnt == 3).all() and (np.sort(idx[:, :3], axis=1) == np.arange(3)).all()):
                failures.append((name, "not one shared set"))
        if name.startswith("n=") and call[0] == "knn" and np.isinf(call[2]):
            n = len(x)
            if not (cnt == min(n, call[1])).all():
                failures.append((name, "m != min(n, k)"))
        if name.startswith("plane lattice"):
            z = np.abs(nrm[:, 2].astype(np.float64))
            if not ((np.abs(R.lam[:, 0]) <= 1e-12 * R.tr).all() and (1 - z <= 8 * nr.U).all() and (np.abs(cur) <= 2 * nr.U).all()):      # (what the bounds come to on an exact plane)
                failures.append((name, "not the plane's normal"))
        if name == "line":
            if not (R.lam[:, 1] <= 1e-12 * R.lam[:, 2]).all():
                failures.append((name, "not a line"))
        if name == "two repeated points":
            if not ((R.tr == 0).all() and np.isnan(cur).all() and np.isfinite(nrm).all() and res["curvature where trace == 0"]["rows"] == 32):
                failures.append((name, "trace == 0 rows"))
        if name == "doubled frame points":
            if not (d2[:, 1] == 0).all():
                failures.append((name, "no distance-0 ties"))
    x, interior = nr.strict_lattice()
    for name, _, call, _ in nr.strict_cases():
        idx, cnt, d2 = nr.oracle_lists(orc, x, call)
        R = nr.reference(x, idx, cnt)
        at = "at the spacing" in name
        if not (cnt[interior] == (9 if at else 11)).all():
            failures.append((name, "interior counts", np.unique(cnt[interior]).tolist()))
        want = 0.0 if at else 4.5 / 16.5
        if not (np.abs(R.curv[interior] - want) <= 1e-15).all():
            failures.append((name, "interior curvature"))
        if at and not (np.abs(np.abs(R.v0[interior][:, 2]) - 1) <= 1e-15).all():
            failures.append((name, "interior normal"))
    assert seen == len(nr.EDGE_SIZES) * (2 * len(nr.EDGE_KS) + 1) + 5 + 4
    assert not failures, failures


def test_the_checks_report_injected_faults(orc, p1):
    _, x, call, vp = nr.frame_cases(p1)[0]
    idx, cnt, d2, R = _case(orc, "knn10", x, call)
    nrm, cur = emulate(x, idx, cnt, vp)
    assert not nr.violations(nr.check(R, nrm, cur, x, vp))
    # rows with a clear gap, a neighbourhood that is no exact plane (so that one neighbour matters) and a view point well off the tangent plane
    to_vp = vp[None, :].astype(np.float64) - x
    cosv = np.abs((nrm * to_vp).sum(axis=1)) / np.linalg.norm(to_vp, axis=1)
    good = np.nonzero((cnt == 10) & ((R.lam[:, 1] - R.lam[:, 0]) > 0.2 * R.tr) & (R.curv > 1e-3) & (cosv > 0.3))[0]
    assert len(good) > 1000
    rows = good[[0, len(good) // 2, -1]]
    for r in rows:
        r = int(r)
        # the last neighbour dropped from the emulation
        c2 = cnt.copy(); c2[r] -= 1
        i2 = idx.copy(); i2[r, cnt[r] - 1] = -1
        n2, k2 = emulate(x, i2, c2, vp)
        assert np.array_equal(np.delete(n2, r, 0), np.delete(nrm, r, 0), equal_nan=True)
        v = nr.violations(nr.check(R, n2, k2, x, vp))
        assert v and all(first == [r] for _, _, _, first in v), ("dropped neighbour", r, v)
        assert {"angle", "curvature"} <= {name for name, _, _, _ in v}, v
        # a wrong neighbour swapped in: the point two places down the k = 32 list is not among the ten nearest
        far = int(np.setdiff1d(np.argsort(((x - x[r]) ** 2).sum(axis=1))[:40], idx[r])[0])
        i3 = idx.copy(); i3[r, cnt[r] - 1] = far
        n3, k3 = emulate(x, i3, cnt, vp)
        v = nr.violations(nr.check(R, n3, k3, x, vp))
        assert v and all(first == [r] for _, _, _, first in v), ("wrong neighbour", r, v)
        # the normal turned away from the view point
        n4 = nrm.copy(); n4[r] = -n4[r]
        v = nr.violations(nr.check(R, n4, cur, x, vp))
        assert [(name, first) for name, _, _, first in v] == [("view point", [r])], ("negated", r, v)
        assert not nr.violations(nr.check(R, n4, cur))
    # the NaN pattern: a NaN where there are neighbours, a number where there are none
    n5 = nrm.copy(); n5[int(rows[0]), 1] = np.nan
    assert "nan pattern" in {name for name, _, _, _ in nr.violations(nr.check(R, n5, cur, x, vp))}
    idx12, cnt12, _, R12 = _case(orc, "knn12_in_radius", x, nr.frame_cases(p1)[2][2])
    n6, k6 = emulate(x, idx12, cnt12, vp)
    lone = int(np.nonzero(cnt12 < 3)[0][0])
    n6[lone] = [0.0, 0.0, 1.0]
    assert [(name, first) for name, _, _, first in nr.violations(nr.check(R12, n6, k6, x, vp))] == [("nan pattern", [lone])]


def test_csr_lists_and_padded_lists_give_the_same_reference(orc, p1):
    x = nr.edge_cloud(p1, 513)
    _, d2_3, cnt_3 = orc.knn_batch(orc.KDTree(x), x, 3, np.inf)
    r2 = np.float32(4.0) * nr.edge_radius_sq(d2_3, cnt_3)
    off, ind, dd = orc.radius_search(x, x, r2)
    idx, cnt, d2 = nr.padded_from_csr(off, ind, dd)
    assert cnt.max() < 64 and (cnt >= 3).any()
    ki, kd, kc = orc.knn_batch(orc.KDTree(x), x, 64, r2)
    assert np.array_equal(kc, cnt) and np.array_equal(np.sort(ki[:, : idx.shape[1]], axis=1), np.sort(idx, axis=1))
    A, B = nr.reference_csr(x, off, ind), nr.reference(x, ki, kc)
    assert np.array_equal(A.m, B.m) and np.allclose(A.lam, B.lam, rtol=1e-12, atol=0, equal_nan=True) and np.allclose(A.Eb, B.Eb, rtol=1e-12, atol=0, equal_nan=True)
