"""NormalEstimation3f on the GPU (k_knn with do_pca, k_radius_pca): EVERY returned normal and curvature against the float64 PCA of
the CPU oracle's neighbour list, inside the a-priori per-row bound of tests/_normal_refs.py (derived from the kernel's documented
arithmetic; tests/test_normal_refs_cpu.py shows that a numpy restatement of that arithmetic meets it on every input used here).
No share of rows is left out: the only conditions are m >= 3, l1 > l0 for the angle and tr > 2 sqrt(3) Eb for the curvature.

The clouds are the ones whose distances tie -- the reference's own sensor frame (more than half of its k = 10 lists hold equal
distances, so the PCA runs behind the second search by position, the refill of a tied k-th place, the reordering of equal-distance
groups and the position-to-index rewrite), doubled points, lattices --, sizes at the 64- and 256-lane edges, k = 3 and 32, k above
the cloud size, neighbourhoods of fewer than 3 points, exact planes, a line, repeated points, the strict '<' of the radius, device
input, the normals-only / curvature-only calls and a view point inside the tangent plane.

Every test writes its figures as normals_*.json (_report): per case the rows checked, the rows with m < 3, the rows whose oracle list
holds equal distances and, per check, the violation count and the worst ratio of value to bound."""
import numpy as np
import pytest

import _normal_refs as nr
from test_gpu_parity import _report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def p1():
    return nr.frame()


_cache = {}


def _lists(orc, tag, x, call):
    """the oracle's lists and the reference on them, computed once per (cloud tag, call)"""
    key = (tag, call)
    if key not in _cache:
        idx, cnt, d2 = nr.oracle_lists(orc, x, call)
        _cache[key] = (idx, cnt, d2, nr.reference(x, idx, cnt))
    return _cache[key]


def _run(x, call, vp, curvature=True):
    """the call under test, squared radii passed as they are -> (normals, curvature or None)"""
    from cilantro_amd.normal_estimation import NormalEstimation3f

    ne = NormalEstimation3f(x).setViewPoint(vp)
    if call[0] == "knn":
        return ne._run(call[1], float(call[2]), curvature)
    return ne._run_radius(float(call[1]), curvature)


def _checked(orc, tag, name, x, call, vp, report, failures, got=None):
    idx, cnt, d2, R = _lists(orc, tag, x, call)
    nrm, cur = _run(x, call, vp) if got is None else got
    res = nr.check(R, nrm, cur, x, vp)
    report[name] = nr.summary(R, res, d2, cnt)
    for v in nr.violations(res):
        failures.append((name,) + v)
    return nrm, cur, R, cnt


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# --------------------------------------------------------------------------------------------------------------------------------
# (a) the sensor frame
# --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ("knn10", "knn32", "knn12_in_radius", "radius", "knn10_no_view_point", "knn10_moved"))
def test_sensor_frame(orc, hip_lib, p1, tag):
    """frame_1 (120 111 points), view point = the sensor: the public calls getNormalsAndCurvatureKNN(10 / 32),
    ...KNNInRadius(12, 0.004) (40 rows with m < 3, 6 067 with m < k), ...Radius(0.004); k = 10 without a view point and moved to
    (1e3, -250, 37) with the view point moved along"""
    from cilantro_amd.normal_estimation import NormalEstimation3f

    _, x, call, vp = next(c for c in nr.frame_cases(p1) if c[0] == tag)
    ne = NormalEstimation3f(x).setViewPoint(vp)
    if call[0] == "radius":
        got = ne.getNormalsAndCurvatureRadius(0.004)
    elif np.isinf(call[2]):
        got = ne.getNormalsAndCurvatureKNN(call[1])
    else:
        got = ne.getNormalsAndCurvatureKNNInRadius(call[1], 0.004)
    report, failures = {}, []
    cloud = "frame moved" if tag == "knn10_moved" else "frame"
    _, _, R, cnt = _checked(orc, cloud, tag, x, call, vp, report, failures, got)
    tied = report[tag]["rows whose list holds equal distances"]
    if tag == "knn10":
        if not (tied == 62974 and tied * 3 > len(x)):
            failures.append((tag, "the oracle's lists no longer tie", tied))
    if tag == "knn12_in_radius" and not ((cnt < 3).sum() == 40 and (cnt < 12).sum() == 6067):
        failures.append((tag, "short rows", int((cnt < 3).sum()), int((cnt < 12).sum())))
    if tag == "radius" and not (cnt < 3).sum() == 40:
        failures.append((tag, "short rows", int((cnt < 3).sum())))
    report["failures"] = [str(f) for f in failures]
    _report(f"normals_frame_{tag}.json", report)
    assert not failures, failures


def test_sensor_frame_tie_rules_1_and_2_agree(orc, hip_lib, p1):
    """k = 10 on the frame under set_knn_tie_rule(1) (order tables built up front): byte for byte what rule 2 returns, and inside the bounds"""
    from cilantro_amd.normal_estimation import NormalEstimation3f, set_knn_tie_rule

    _, x, call, vp = nr.frame_cases(p1)[0]
    ne = NormalEstimation3f(x).setViewPoint(vp)
    n2, c2 = ne.getNormalsAndCurvatureKNN(10)
    set_knn_tie_rule(1)
    try:
        n1, c1 = ne.getNormalsAndCurvatureKNN(10)
    finally:
        set_knn_tie_rule(2)
    report, failures = {}, []
    _checked(orc, "frame", "rule 1", x, call, vp, report, failures, (n1, c1))
    report["byte-identical to rule 2"] = {"normals": _same(n1, n2), "curvature": _same(c1, c2)}
    if not (_same(n1, n2) and _same(c1, c2)):
        failures.append(("rule 1 differs from rule 2", int(np.count_nonzero((n1.view(np.uint32) != n2.view(np.uint32)).any(axis=1)))))
    report["failures"] = [str(f) for f in failures]
    _report("normals_frame_tie_rule_1.json", report)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------------------------
# (b) block and wave edges
# --------------------------------------------------------------------------------------------------------------------------------

def test_block_and_wave_edges(orc, hip_lib, p1):
    """the first n points of the shuffled frame, n at the 64- and 256-lane edges and down to 3, k in (3, 10, 32) (k > n: m = n): plain
    k-NN, k-NN inside a radius that leaves some rows under 3 members, and that radius alone.  n = 3, k = 3: the three rows share one
    exactly planar set -- the Rayleigh bound holds the normal to the triangle's plane."""
    report, failures = {}, []
    tri = None
    for name, x, call, vp in nr.edge_cases(orc, p1):
        nrm, _, R, cnt = _checked(orc, f"edge {len(x)}", name, x, call, vp, report, failures)
        if name == "n=3/knn 3":
            t = np.cross(x[1].astype(np.float64) - x[0], x[2].astype(np.float64) - x[0])
            tri = [float(np.linalg.norm(np.cross(r.astype(np.float64), t / np.linalg.norm(t)))) for r in nrm]
        if "radius" in name and not (cnt < 3).any():
            failures.append((name, "no row under 3 members"))
        if call[0] == "knn" and np.isinf(call[2]) and not (cnt == min(len(x), call[1])).all():
            failures.append((name, "m != min(n, k)"))
    report["n=3, k=3: |n x triangle normal|"] = tri
    report["failures"] = [str(f) for f in failures]
    _report("normals_edges.json", report)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------------------------
# (c) constructed degenerate neighbourhoods
# --------------------------------------------------------------------------------------------------------------------------------

def test_degenerate_neighbourhoods(orc, hip_lib, p1):
    """dyadic coordinates (exact f32 inputs): a 32 x 32 lattice in the plane z = 4096.5 (every normal within its bound of (0, 0, +-1),
    curvature within its bound of 0; once with the view point inside that plane), 40 points on a line (the Rayleigh bound holds the
    component along the line), 16 + 16 copies of two points (trace == 0 exactly: normal finite and unit, curvature NaN = 0 / 0) and
    5 000 frame points doubled (distance-0 ties)."""
    report, failures = {}, []
    for name, x, call, vp in nr.degenerate_cases(p1):
        nrm, cur, R, cnt = _checked(orc, name, name, x, call, vp, report, failures)
        if name.startswith("plane lattice"):
            if not ((1 - np.abs(R.v0[:, 2]) <= 1e-15).all() and (np.abs(R.lam[:, 0]) <= 1e-12 * R.tr).all()):
                failures.append((name, "the reference is not the plane"))
        if name == "line":
            along = np.abs(nrm.astype(np.float64) @ (np.array([1.0, 1.0, 2.0]) / np.sqrt(6.0)))
            report[name]["largest component along the line"] = float(along.max())
            if not (R.lam[:, 1] <= 1e-12 * R.lam[:, 2]).all():
                failures.append((name, "the reference is not a line"))
        if name == "two repeated points":
            finite_unit = bool(np.isfinite(nrm).all() and (np.abs(np.linalg.norm(nrm.astype(np.float64), axis=1) - 1) <= 4 * nr.U).all())
            report[name]["normals finite and unit"] = finite_unit
            report[name]["curvature all NaN"] = bool(np.isnan(cur).all())
            report[name]["distinct normals"] = np.unique(nrm, axis=0).tolist()
            if not ((R.tr == 0).all() and report[name]["checks"]["curvature where trace == 0"]["rows"] == len(x)):
                failures.append((name, "the reference's trace is not 0"))
            if not (finite_unit and np.isnan(cur).all()):
                failures.append((name, "normal not finite and unit, or curvature not NaN"))
        if name == "doubled frame points":
            if not report[name]["rows whose list holds equal distances"] == len(x):
                failures.append((name, "no distance-0 ties"))
    report["failures"] = [str(f) for f in failures]
    _report("normals_degenerate.json", report)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------------------------
# (d) the strict radius
# --------------------------------------------------------------------------------------------------------------------------------

def test_strict_radius(orc, hip_lib):
    """lattice g (h, h, 1.5 h) + (8, -8, 4), h = 2^-6: at radius_sq = float32(9 2^-14), the squared z spacing itself, an interior
    point has exactly 9 neighbours, all in its own z layer (normal within its bound of (0, 0, +-1), curvature of 0); one ulp above it
    has 11 and the curvature follows 4.5 / 16.5.  Both squared radii go to cilhip_normals_radius3f and to cilhip_normals_knn3f
    (k = 32) as they are, not through a square root."""
    x, interior = nr.strict_lattice()
    report, failures = {}, []
    for name, _, call, vp in nr.strict_cases():
        nrm, cur, R, cnt = _checked(orc, "strict lattice", name, x, call, vp, report, failures)
        at = "at the spacing" in name
        want_m, want_c = (9, 0.0) if at else (11, 4.5 / 16.5)
        if not ((cnt[interior] == want_m).all() and (np.abs(R.curv[interior] - want_c) <= 1e-15).all()):
            failures.append((name, "the reference's interior neighbourhoods", np.unique(cnt[interior]).tolist()))
        if at and not (1 - np.abs(R.v0[interior][:, 2]) <= 1e-15).all():
            failures.append((name, "the reference's interior normal"))
        report[name]["interior: largest |curvature - %.6g|" % want_c] = float(np.abs(cur[interior].astype(np.float64) - want_c).max())
        report[name]["interior: smallest |n_z|"] = float(np.abs(nrm[interior][:, 2]).min())
    report["failures"] = [str(f) for f in failures]
    _report("normals_strict_radius.json", report)
    assert not failures, failures


# --------------------------------------------------------------------------------------------------------------------------------
# (e) entry points
# --------------------------------------------------------------------------------------------------------------------------------

def _entry_point_equalities(x, vp, k, radius, failures, tag):
    import torch

    from cilantro_amd.normal_estimation import NormalEstimation3f

    ne = NormalEstimation3f(x).setViewPoint(vp)
    xd = torch.from_numpy(x).cuda()
    forms = (("KNN", (k,)), ("KNNInRadius", (k, radius)), ("Radius", (radius,)))
    out = {}
    for form, args in forms:
        nrm, cur = getattr(ne, f"getNormalsAndCurvature{form}")(*args)
        eq = {"normals-only call": _same(getattr(ne, f"getNormals{form}")(*args), nrm),
              "curvature-only call": _same(getattr(ne, f"getCurvature{form}")(*args), cur)}
        nd, cd = getattr(NormalEstimation3f(xd).setViewPoint(vp), f"getNormalsAndCurvature{form}")(*args)
        eq["device input"] = _same(nd, nrm) and _same(cd, cur)
        n2, c2 = getattr(ne, f"getNormalsAndCurvature{form}")(*args)
        eq["second run"] = _same(n2, nrm) and _same(c2, cur)
        nn, cn = getattr(NormalEstimation3f(x).setViewPoint(None), f"getNormalsAndCurvature{form}")(*args)
        nv, cv = getattr(NormalEstimation3f(x).setViewPoint([np.nan, 0.0, 0.0]), f"getNormalsAndCurvature{form}")(*args)
        eq["NaN view point = no view point"] = _same(nv, nn) and _same(cv, cn)
        eq["rows with a normal"] = int((~np.isnan(nrm).any(axis=1)).sum())
        out[form] = eq
        for what, same in eq.items():
            if same is False:
                failures.append((tag, form, what))
        if not 0 < eq["rows with a normal"]:
            failures.append((tag, form, "nothing compared"))
    return out


def test_entry_points_agree_byte_for_byte(orc, hip_lib, p1):
    """getNormals* and getCurvature* against the with-curvature calls, a torch device tensor against the host array, a NaN view point
    against none, and a second run of the same call: identical bytes, on the 257-point cloud of the edge cases and on the frame"""
    failures = []
    x = nr.edge_cloud(p1, 257)
    _, d2_3, cnt_3 = orc.knn_batch(orc.KDTree(x), x, 3, np.inf)
    report = {"257 points": _entry_point_equalities(x, np.float32([0.1, -0.2, 0.05]), 10, float(np.sqrt(np.float32(4.0) * nr.edge_radius_sq(d2_3, cnt_3))), failures, "257 points"),
              "frame": _entry_point_equalities(p1, np.zeros(3, np.float32), 10, 0.004, failures, "frame")}
    report["failures"] = [str(f) for f in failures]
    _report("normals_entry_points.json", report)
    assert not failures, failures
