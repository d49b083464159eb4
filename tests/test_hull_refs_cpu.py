"""CPU: the yardstick of DESIGN.md section 20 and everything of the convex hull that needs no device.
  * the fixtures of tests/_hull_refs.py keep clear of the band under scipy alone, and _hull_refs' area / volume sums agree with scipy's
  * csrc/hull_host.hpp (tests/cpp/test_hull_host.cpp, a stand-alone program; built a second time under ASan / UBSan) gives the
    reference's vertex and facet lists on every fixture
  * the argument rules of the six entries, and the empty polytope for n == 0, without a device
  * the spatial.py and spatial.hpp mirrors' host halves
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _hull_refs as R
from test_components_refs_cpu import build_cpp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLEAR = ["gauss65537", "offset_aniso65537", "sphere3000", "unit257"]


# ---- the yardstick itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLEAR)
def test_fixture_keeps_clear_of_the_band(name):
    """a condition on the INPUT: every non-vertex lies more than 1000 tol below every facet, every vertex more than 1000 tol below every
    facet it is not part of.  If a seed ever fails this, change the seed."""
    pts = R.fixture(name).astype(np.float64)
    ref = R.ref_of(name)
    tol = ref["tol"]
    is_vertex = np.zeros(len(pts), bool)
    is_vertex[ref["vertex_point_indices"]] = True
    incident = np.zeros((len(ref["facets"]), len(ref["vertex_point_indices"])), bool)
    for k, f in enumerate(ref["facets"]):
        incident[k, f] = True
    nonvertex_clear, vertex_clear = np.inf, np.inf
    for c in range(0, len(ref["planes"]), 256):
        d = R.dist_all(ref["planes"][c:c + 256], pts)
        if (~is_vertex).any():
            nonvertex_clear = min(nonvertex_clear, float(-d[:, ~is_vertex].max()))
        dv = d[:, ref["vertex_point_indices"]]
        dv[incident[c:c + 256]] = -np.inf
        vertex_clear = min(vertex_clear, float(-dv.max()))
    print(name, "non-vertex clearance", nonvertex_clear, "vertex clearance", vertex_clear, "tol", tol)
    assert nonvertex_clear > 1000 * tol
    assert vertex_clear > 1000 * tol


@pytest.mark.parametrize("name", CLEAR + ["gauss2d_65537"])
def test_sums_agree_with_scipy(name):
    ref = R.ref_of(name)
    vb, ab = R.sum_bounds(R.fixture(name), len(ref["facets"]))
    print(name, "volume", abs(ref["volume"] - ref["scipy_volume"]), vb, "area", abs(ref["area"] - ref["scipy_area"]), ab)
    assert abs(ref["volume"] - ref["scipy_volume"]) <= vb
    assert abs(ref["area"] - ref["scipy_area"]) <= ab
    # dropping one facet moves either sum by orders of magnitude more
    assert ref["area"] / len(ref["facets"]) > 1e4 * ab


def test_cube12_reference():
    tri, quad = R.ref_of("cube12", True), R.ref_of("cube12", False)
    assert tri["vertex_point_indices"].tolist() == list(range(8)) == quad["vertex_point_indices"].tolist()
    assert len(tri["facets"]) == 12 and len(quad["facets"]) == 6 and all(len(f) == 4 for f in quad["facets"])
    assert tri["volume"] == quad["volume"] == 1.0 and tri["area"] == quad["area"] == 6.0
    for name in R.DEGENERATE:
        assert R.ref_of(name)["is_empty"], name


# ---- hull_host.hpp on its own ---------------------------------------------------------------------------------------
def _parse(out):
    lines = out.splitlines()
    head = lines[0].split()
    got = dict(is_empty=bool(int(head[1])), failed=bool(int(head[3])), n_nonfinite=int(head[5]))
    if not got["is_empty"]:
        got["vertices"] = [int(x) for x in lines[1].split()[1:]]
        got["facets"] = [[int(x) for x in l.split()[1:]] for l in lines if l.startswith("F")]
        got["neighbors"] = [[int(x) for x in l.split()[1:]] for l in lines if l.startswith("N")]
        got["area"], got["volume"] = (float(x) for x in lines[-1].split()[1:])
    return got


HOST_CASES = [(n, 1) for n in R.ALL_3D + R.ALL_2D + R.DEGENERATE + ["big"]] + [("demo9", 0), ("cube12", 0)]


@pytest.fixture(scope="module")
def host_binaries(tmp_path_factory):
    src = os.path.join(HERE, "cpp", "test_hull_host.cpp")
    plain = build_cpp(src, "test_hull_host")
    san = os.path.join(os.path.dirname(plain), "test_hull_host_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", san],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return plain, san, tmp_path_factory.mktemp("hull_raw")


@pytest.mark.parametrize("name,simplicial", HOST_CASES)
def test_host_builder_equals_the_reference(host_binaries, name, simplicial):
    plain, san, tmp = host_binaries
    pts = R.fixture(name)
    raw = os.path.join(str(tmp), name + ".raw")
    pts.tofile(raw)
    ref = R.ref_of(name, bool(simplicial))
    for exe in (plain, san):
        r = subprocess.run([exe, raw, str(len(pts)), str(pts.shape[1]), str(simplicial)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[:300] + r.stderr[-2000:]
        got = _parse(r.stdout)
        assert not got["failed"] and got["is_empty"] == ref["is_empty"] and got["n_nonfinite"] == ref["n_nonfinite"]
        if ref["is_empty"]:
            continue
        assert got["vertices"] == ref["vertex_point_indices"].tolist()
        assert got["facets"] == ref["facets"]
        assert got["neighbors"] == ref["facet_neighbors"]
        vb, ab = R.sum_bounds(pts, len(ref["facets"]))
        assert abs(got["volume"] - ref["scipy_volume"]) <= vb and abs(got["area"] - ref["scipy_area"]) <= ab


# ---- argument rules, without a device -------------------------------------------------------------------------------
def _err(L):
    return L.cilhip_last_error(None).decode()


def test_hull_argument_rules(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    pts = np.zeros((8, 3), np.float32)
    h, info = C.c_void_p(), capi.HullInfo()

    def call(points=pts.ctypes.data, n=8, dim=3, mem=0, tol=0.0, out=C.byref(h), inf=C.byref(info)):
        return L.cilhip_convex_hull_create(0, points, n, dim, mem, 1, tol, out, inf)

    for kwargs, needle in ((dict(points=None), "points is NULL"), (dict(out=None), "out or info is NULL"), (dict(inf=None), "out or info is NULL"), (dict(dim=1), "dim must be 2 or 3"),
                           (dict(dim=4), "dim must be 2 or 3"), (dict(n=2 ** 32 - 16), "2^32 - 16"), (dict(mem=2), "mem"), (dict(tol=-1.0), "merge_tol"),
                           (dict(tol=float("nan")), "merge_tol"), (dict(tol=float("inf")), "merge_tol")):
        assert call(**kwargs) == capi.ERR_INVALID, kwargs
        assert needle in _err(L) and _err(L).startswith("convex_hull: "), (kwargs, _err(L))
        assert not h.value
    assert L.cilhip_convex_hull_get(None, None, None, None, None, None, None, None, None, None) == capi.ERR_INVALID


@pytest.mark.parametrize("dim", [2, 3])
def test_n_zero_is_the_empty_polytope_without_a_device(hip_lib, dim):
    from cilantro_amd import capi

    h, info = C.c_void_p(), capi.HullInfo()
    assert hip_lib.cilhip_convex_hull_create(0, None, 0, dim, 0, 1, 0.0, C.byref(h), C.byref(info)) == capi.OK
    assert info.is_empty == 1 and info.dim == dim and info.n_vertices == 0 and info.n_facets == 0 and info.n_halfspaces == 2 and info.area == 0.0 and info.volume == 0.0
    assert info.rounds == 0 and all(np.isnan(info.interior_point[c]) for c in range(dim))
    hs = np.zeros((2, dim + 1), np.float32)
    fo = np.full(1, 9, np.uint32)
    assert hip_lib.cilhip_convex_hull_get(h, None, None, hs.ctypes.data, fo.ctypes.data, None, None, None, None, None) == capi.OK
    hip_lib.cilhip_convex_hull_destroy(h)
    want = R.empty_hull(dim)["halfspaces"]
    assert np.array_equal(hs.T, want) and fo[0] == 0


def test_query_argument_rules(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    hs = np.zeros((6, 4), np.float32)
    pts = np.zeros((5, 3), np.float32)
    out = np.zeros(64, np.float32)
    good = np.array([0, 2, 6], np.uint32)
    count = C.c_size_t(77)

    def mask(hsp=hs.ctypes.data, po=good.ctypes.data, npoly=2, p=pts.ctypes.data, n=5, dim=3, mem=0, offset=0.0, o=out.ctypes.data):
        return L.cilhip_polytopes_interior_mask(0, hsp, po, npoly, p, n, dim, mem, C.c_float(offset), o)

    def indices(hsp=hs.ctypes.data, po=good.ctypes.data, npoly=2, p=pts.ctypes.data, n=5, dim=3, mem=0, offset=0.0, o=out.ctypes.data, cap=5, cnt=C.byref(count)):
        return L.cilhip_polytopes_interior_indices(0, hsp, po, npoly, p, n, dim, mem, C.c_float(offset), o, cap, cnt)

    def dist(hsp=hs.ctypes.data, F=6, p=pts.ctypes.data, n=5, dim=3, mem=0, o=out.ctypes.data):
        return L.cilhip_polytope_signed_distances(0, hsp, F, p, n, dim, mem, o)

    bad_start, descending = np.array([1, 2, 6], np.uint32), np.array([0, 4, 2], np.uint32)
    for fn, family in ((mask, "polytopes_interior_mask"), (indices, "polytopes_interior_indices")):
        for kwargs, needle in ((dict(po=None), "poly_offsets is NULL"), (dict(p=None), "points is NULL"), (dict(hsp=None), "halfspaces is NULL"), (dict(dim=4), "dim must be 2 or 3"),
                               (dict(n=2 ** 32 - 16), "2^32 - 16"), (dict(mem=3), "mem"), (dict(po=bad_start.ctypes.data), "ascend from 0"),
                               (dict(po=descending.ctypes.data), "ascend from 0"), (dict(offset=float("nan")), "offset is NaN"), (dict(o=None), "is NULL")):
            assert fn(**kwargs) == capi.ERR_INVALID, (family, kwargs)
            assert needle in _err(L) and _err(L).startswith(family + ": "), (kwargs, _err(L))
    assert indices(cnt=None) == capi.ERR_INVALID and "n_out is NULL" in _err(L)
    for kwargs, needle in ((dict(hsp=None), "halfspaces is NULL"), (dict(p=None), "points is NULL"), (dict(o=None), "out is NULL"), (dict(dim=1), "dim must be 2 or 3"),
                           (dict(n=2 ** 32 - 16), "2^32 - 16"), (dict(mem=-1), "mem")):
        assert dist(**kwargs) == capi.ERR_INVALID, kwargs
        assert needle in _err(L) and _err(L).startswith("polytope_signed_distances: "), (kwargs, _err(L))
    # no points: nothing to do, no device needed
    assert mask(n=0) == capi.OK and dist(n=0) == capi.OK
    assert indices(n=0) == capi.OK and count.value == 0


# ---- the mirrors' host halves ---------------------------------------------------------------------------------------
def _cube_hs():
    return R.ref_of("demo9", False)["halfspaces"]


def test_spatial_py_contains_and_transform_against_numpy(hip_lib):
    from cilantro_amd import capi, spatial

    rng = np.random.default_rng(11)
    hs = R.ref_of("unit257")["halfspaces"]
    poly = spatial.ConvexPolytope3f.from_halfspaces(hs)
    pts = np.concatenate([rng.uniform(-0.2, 1.2, (300, 3)).astype(np.float32), R.ref_of("unit257")["vertices"]])
    for offset in (0.0, 0.01, -0.01):
        want = R.ref_mask((hs,), pts, offset)
        assert [poly.containsPoint(p, offset) for p in pts] == want.tolist()
        assert want.any() and not want.all()
    # transform: the halfspaces by [[R, 0], [-t^T R, 1]] in f32 (convex_polytope.hpp:155-174)
    a = 0.3
    Rm = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
    t = np.array([0.5, -2.0, 3.0], np.float32)
    H = np.zeros((4, 4), np.float32)
    H[:3, :3], H[3, :3], H[3, 3] = Rm, -(t @ Rm), 1.0
    moved = poly.transformed(Rm, t)
    exact = H.astype(np.float64) @ hs.astype(np.float64)      # four f32 products and three sums per entry: a few ulp of the largest term
    assert np.abs(moved.getFacetHyperplanes() - exact).max() <= 8 * 2.0 ** -24 * (np.abs(H).astype(np.float64) @ np.abs(hs).astype(np.float64)).max()
    assert np.array_equal(poly.getFacetHyperplanes(), hs)      # transformed() copies
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = Rm, t
    assert np.array_equal(poly.transformed(T).getFacetHyperplanes(), moved.getFacetHyperplanes())
    # a point and its image agree (away from the boundary)
    inner = pts[R.ref_mask((hs,), pts, 0.01)]
    assert len(inner) > 10 and all(moved.containsPoint(Rm @ p + t) for p in inner)
    region = spatial.SpaceRegion3f([poly]).unionWith(spatial.SpaceRegion3f([moved]))
    assert len(region.getConvexPolytopes()) == 2 and region.containsPoint(inner[0]) and region.containsPoint(Rm @ inner[0] + t) and not region.containsPoint([50, 50, 50])
    # what is not built says so; a polytope given by halfspaces has no vertices
    for fn in (poly.getVertices, poly.intersectionWith, region.complement, region.getVolume, lambda: region.relativeComplement(region), lambda: region.intersectionWith(region)):
        with pytest.raises(capi.CilhipError) as e:
            fn()
        assert e.value.code == capi.ERR_UNSUPPORTED and "convex_hull_utilities.hpp:12-193" in str(e.value)
    # the empty polytope needs no device
    empty = spatial.ConvexPolytope3f()
    assert empty.isEmpty() and len(empty.getVertices()) == 0 and np.isnan(empty.getInteriorPoint()).all() and not empty.containsPoint([0, 0, 0])
    assert np.array_equal(empty.getFacetHyperplanes(), R.empty_hull(3)["halfspaces"])
    assert empty.transform(T) is empty and spatial.SpaceRegion3f([empty]).isEmpty() and np.isnan(spatial.SpaceRegion3f([empty]).getInteriorPoint()).all()
    assert spatial.ConvexHull3f is spatial.ConvexPolytope3f and spatial.ConvexHull2f is spatial.ConvexPolytope2f


def test_cpp_mirror_and_example_compile():
    exe = build_cpp(os.path.join(HERE, "cpp", "test_spatial.cpp"), "test_spatial")
    build_cpp(os.path.join(ROOT, "examples", "convex_hull.cpp"), "example_convex_hull")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "convex_hull.cpp")).read()
    for needle in ("ConvexHull3f ch(points, true)", "ConvexHull3f ch(cloud.points, true, true)", "getVertexPointIndices()"):
        assert needle in src, needle


def test_sources_are_registered():
    from cilantro_amd import build

    assert "convex_hull.hip" in build.SOURCES and "polytope_query.hip" in build.SOURCES and "hull_host.hpp" in build.HEADERS
    host = open(os.path.join(ROOT, "cilantro_amd", "csrc", "hull_host.hpp")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host      # plain C++
