"""GPU: cilhip_convex_hull_* and the spatial.py mirror against tests/_hull_refs.py (scipy.spatial.ConvexHull in the canonical order of
DESIGN.md section 20).  Integer outputs are compared exactly, halfspaces and the interior point bit for bit, area and volume within the
rounding bounds _hull_refs.sum_bounds states."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _hull_refs as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def capi_hull(points, simplicial=True, mem="host", merge_tol=0.0):
    """-> (dict in _hull_refs' shape, info dict)"""
    import torch

    from cilantro_amd import capi

    L = capi.load()
    pts = np.ascontiguousarray(points, np.float32)
    n, dim = pts.shape
    if mem == "device":
        t = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        ptr, m = t.data_ptr(), capi.MEM_DEVICE
    else:
        ptr, m = pts.ctypes.data, capi.MEM_HOST
    h, info = C.c_void_p(), capi.HullInfo()
    rc = L.cilhip_convex_hull_create(0, ptr, n, dim, m, int(simplicial), merge_tol, C.byref(h), C.byref(info))
    assert rc == capi.OK, L.cilhip_last_error(None).decode()
    V, F = info.n_vertices, info.n_facets
    vpi, verts, hs = np.zeros(V, np.uint32), np.zeros((V, dim), np.float32), np.zeros((info.n_halfspaces, dim + 1), np.float32)
    fo, fi, fn = np.zeros(F + 1, np.uint32), np.zeros(info.n_facet_indices, np.uint32), np.zeros(info.n_facet_indices, np.uint32)
    vo, vf = np.zeros(V + 1, np.uint32), np.zeros(info.n_vertex_facets, np.uint32)
    surv = np.zeros(info.rounds, np.uint64)
    assert L.cilhip_convex_hull_get(h, vpi.ctypes.data, verts.ctypes.data, hs.ctypes.data, fo.ctypes.data, fi.ctypes.data, fn.ctypes.data, vo.ctypes.data, vf.ctypes.data,
                                    surv.ctypes.data) == capi.OK
    L.cilhip_convex_hull_destroy(h)
    got = dict(dim=dim, is_empty=bool(info.is_empty), vertex_point_indices=vpi, vertices=verts, facets=[fi[fo[k]:fo[k + 1]].tolist() for k in range(F)],
               facet_neighbors=[fn[fo[k]:fo[k + 1]].tolist() for k in range(F)], vertex_facets=[vf[vo[k]:vo[k + 1]].tolist() for k in range(V)],
               halfspaces=np.ascontiguousarray(hs.T), interior_point=np.array(info.interior_point[:dim], np.float32), area=info.area, volume=info.volume,
               n_nonfinite=info.n_nonfinite, raw=(vpi, verts, hs, fo, fi, fn, vo, vf, surv))
    inf = {k: getattr(info, k) for k, _ in capi.HullInfo._fields_ if k not in ("interior_point", "cull_ms")}
    return got, inf


def mirror_hull(points, simplicial=True, mem="host"):
    import torch

    from cilantro_amd import spatial

    pts = np.ascontiguousarray(points, np.float32)
    cls = spatial.ConvexHull3f if pts.shape[1] == 3 else spatial.ConvexHull2f
    hull = cls(torch.from_numpy(pts).cuda() if mem == "device" else pts, True, simplicial)
    got = dict(dim=pts.shape[1], is_empty=hull.isEmpty(), vertex_point_indices=hull.getVertexPointIndices(), vertices=hull.getVertices(), facets=hull.getFacetVertexIndices(),
               facet_neighbors=hull.getFacetNeighborFacets(), vertex_facets=hull.getVertexNeighborFacets(), halfspaces=np.ascontiguousarray(hull.getFacetHyperplanes()),
               interior_point=hull.getInteriorPoint(), area=hull.getArea(), volume=hull.getVolume(), n_nonfinite=hull.info_["n_nonfinite"])
    return got, hull.info_


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check(got, ref, pts):
    assert got["is_empty"] == ref["is_empty"]
    assert got["n_nonfinite"] == ref["n_nonfinite"]
    assert np.array_equal(got["vertex_point_indices"], ref["vertex_point_indices"])
    assert np.array_equal(bits(got["halfspaces"]), bits(ref["halfspaces"]))
    if ref["is_empty"]:
        assert got["facets"] == [] and got["vertices"].shape[0] == 0 and got["area"] == 0.0 and got["volume"] == 0.0
        assert np.isnan(got["interior_point"]).all()
        return
    assert got["facets"] == ref["facets"]
    assert got["facet_neighbors"] == ref["facet_neighbors"]
    assert got["vertex_facets"] == ref["vertex_facets"]
    assert np.array_equal(bits(got["vertices"]), bits(ref["vertices"]))
    assert np.array_equal(bits(got["interior_point"]), bits(ref["interior_point"]))
    vb, ab = R.sum_bounds(pts, len(ref["facets"]))
    print("volume", got["volume"] - ref["scipy_volume"], "bound", vb, "area", got["area"] - ref["scipy_area"], "bound", ab)
    assert abs(got["volume"] - ref["scipy_volume"]) <= vb
    assert abs(got["area"] - ref["scipy_area"]) <= ab
    # containment by construction: no input point lies more than tol above an output facet.  The planes are recomputed from the OUTPUT
    vp = [tuple(float(c) for c in row) for row in got["vertices"]]
    if got["dim"] == 3:
        def plane(f):
            best = min(range(1, len(f) - 1), key=lambda i: (min(f[i], f[i + 1]), max(f[i], f[i + 1])))
            return R.plane3(vp[f[0]], vp[f[best]], vp[f[best + 1]])
    else:
        def plane(f):
            return R.plane2(vp[f[0]], vp[f[1]])
    planes = np.array([plane(f) for f in got["facets"]])
    fin = np.asarray(pts, np.float64)
    fin = fin[np.isfinite(fin).all(axis=1)]
    step = max(1, min(256, (1 << 24) // max(len(fin), 1)))      # planes per block: at most 2^24 distances at a time, however many points
    worst = max(float(R.dist_all(planes[c:c + step], fin).max()) for c in range(0, len(planes), step))
    print("largest d", worst, "tol", ref["tol"])
    assert worst <= ref["tol"]


CASES = [(name, True) for name in R.ALL_3D + R.ALL_2D] + [("demo9", False), ("cube12", False)]


@pytest.mark.parametrize("path", ["capi-host", "capi-device", "mirror-host", "mirror-device"])
@pytest.mark.parametrize("name,simplicial", CASES)
def test_hull_equals_the_reference(name, simplicial, path):
    pts = R.fixture(name)
    via, mem = path.split("-")
    got, _ = (capi_hull if via == "capi" else mirror_hull)(pts, simplicial, mem)
    check(got, R.ref_of(name, simplicial), pts)


def test_cube12_is_the_unit_cube():
    for simplicial, n_facets, width in ((True, 12, 3), (False, 6, 4)):
        got, info = capi_hull(R.fixture("cube12"), simplicial)
        assert got["vertex_point_indices"].tolist() == list(range(8))
        assert len(got["facets"]) == n_facets and all(len(f) == width for f in got["facets"])
        assert got["volume"] == pytest.approx(1.0, abs=1e-12) and got["area"] == pytest.approx(6.0, abs=1e-12)


def test_sphere_runs_the_tile_loop_and_several_rounds():
    got, info = capi_hull(R.fixture("sphere3000"))
    assert info["n_facets"] == 5996 and info["n_vertices"] == 3000
    assert info["n_facets"] > 2 * info["facet_tile"]
    assert info["rounds"] >= 2
    surv = got["raw"][8]
    assert len(surv) == info["rounds"] and surv[-1] == 0 and surv[0] == info["survivors_first_round"]


def test_solid_ball_is_culled_to_its_shell():
    pts = R.fixture("shell_solid23000")
    got, info = capi_hull(pts)
    ref = R.ref_of("sphere3000")
    assert np.array_equal(got["vertex_point_indices"], ref["vertex_point_indices"])      # the shell comes first in the fixture
    assert got["facets"] == ref["facets"]
    assert np.array_equal(bits(got["halfspaces"]), bits(ref["halfspaces"]))
    assert info["survivors_first_round"] < len(pts)


def test_big_equals_scipy_and_two_runs_are_identical():
    pts = R.fixture("big")
    a, ia = capi_hull(pts)
    b, ib = capi_hull(pts)
    check(a, R.ref_hull(pts), pts)
    assert ia == ib
    for x, y in zip(a["raw"], b["raw"]):
        assert x.tobytes() == y.tobytes()
    assert (a["area"], a["volume"]) == (b["area"], b["volume"]) and bits(a["interior_point"]).tolist() == bits(b["interior_point"]).tolist()


def test_nonfinite_rows_are_ignored_and_counted():
    pts = R.fixture("nonfinite")
    got, info = capi_hull(pts)
    fin = np.isfinite(pts).all(axis=1)
    assert info["n_nonfinite"] == int((~fin).sum()) == 6
    clean, _ = capi_hull(pts[fin])
    assert np.array_equal(np.nonzero(fin)[0][clean["vertex_point_indices"]], got["vertex_point_indices"])
    assert clean["facets"] == got["facets"] and np.array_equal(bits(clean["halfspaces"]), bits(got["halfspaces"]))


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", R.DEGENERATE)
def test_degenerate_input_gives_the_empty_polytope(name, mem):
    pts = R.fixture(name)
    got, info = capi_hull(pts, True, mem)
    assert R.ref_of(name)["is_empty"]
    check(got, R.ref_of(name), pts)
    assert info["is_empty"] == 1 and info["n_vertices"] == 0 and info["n_facets"] == 0 and info["n_halfspaces"] == 2
    assert got["halfspaces"].T.tolist() == [[1, 0, 0, 1], [-1, 0, 0, 1]]
    if name != "three_points":      # the 2-D image of the same degeneracy
        got2, info2 = capi_hull(np.ascontiguousarray(pts[:, :2] if name != "coplanar300" else np.stack([pts[:, 0], 2 * pts[:, 0]], axis=1)), True, mem)
        assert info2["is_empty"] == 1 and got2["halfspaces"].T.tolist() == [[1, 0, 1], [-1, 0, 1]]


def test_flat_convex_hull():
    from cilantro_amd import spatial
    from cilantro_amd.principal_component_analysis import PrincipalComponentAnalysis

    pts = R.fixture("flat_noisy300")
    flat = spatial.FlatConvexHull3f(pts)
    pca = PrincipalComponentAnalysis(pts)
    proj = pca.project(pts, 2)
    ref2 = R.ref_hull(proj)
    assert np.array_equal(flat.getVertexPointIndices(), ref2["vertex_point_indices"])
    assert flat.getFacetVertexIndices() == ref2["facets"]
    assert np.array_equal(bits(flat.getVertices2D()), bits(proj[ref2["vertex_point_indices"]]))
    assert np.array_equal(bits(flat.getVertices3D()), bits(pca.reconstruct(proj[ref2["vertex_point_indices"]])))
    assert flat.getVertices3D().shape == (len(ref2["vertex_point_indices"]), 3)


def test_example_prints_the_cube():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(ROOT, "examples", "convex_hull.cpp"), "example_convex_hull")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert any(l.strip() == "Vertices: 8" for l in lines), r.stdout
    faces = [l.split(":")[1].split() for l in lines if l.startswith("Face ") and l.split()[1].rstrip(":").isdigit()]
    assert len(faces) == 6 and all(len(f) == 4 for f in faces), r.stdout
