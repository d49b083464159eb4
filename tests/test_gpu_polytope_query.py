"""GPU: cilhip_polytope_signed_distances / cilhip_polytopes_interior_mask / _indices and the SpaceRegion mirror against the numpy f32
restatement of tests/_hull_refs.py (rules Q1, Q2 of c_api.h).  Everything is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest

import _hull_refs as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def cube(shift):
    """the unit cube's six halfspaces (exact in f32), shifted"""
    hs = R.ref_of("demo9", False)["halfspaces"].copy()      # (4, 6)
    hs[3] = hs[3] - (hs[:3] * np.asarray(shift, F32)[:, None]).sum(axis=0)
    return hs.astype(F32)


@functools.lru_cache(maxsize=None)
def region(name):
    """-> tuple of (dim + 1, F_p) f32 arrays"""
    empty = R.empty_hull(3)["halfspaces"]
    if name == "gauss":
        return (R.ref_of("gauss65537")["halfspaces"],)
    if name == "sphere":
        return (R.ref_of("sphere3000")["halfspaces"],)
    if name == "cubes":
        return (cube([0, 0, 0]), cube([0.5, 0.25, 0]), cube([-2, 0, 1]))
    if name == "empty":
        return (empty,)
    if name == "everything":
        return (np.zeros((4, 0), F32),)
    if name == "mixed":      # an empty one first, a hull past the tile in the middle
        return (empty, cube([3, 3, 3]), R.ref_of("sphere3000")["halfspaces"], cube([0, 0, 0]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def queries(name):
    rng = np.random.default_rng(R.hash_name("queries" + name))
    n = 4099 if name in ("sphere", "mixed") else 65537
    pts = (rng.standard_normal((n, 3)) * (0.7 if name in ("sphere", "mixed") else 1.5)).astype(F32)
    if name == "gauss":      # the hull's own vertices
        v = R.ref_of("gauss65537")["vertices"]
        pts[:len(v)] = v
    if name == "sphere":
        pts[:3000] = R.ref_of("sphere3000")["vertices"]
    if name in ("cubes", "mixed"):      # points exactly on faces, edges and corners of the unit cube: v is exactly 0 there
        grid = np.array([[x, y, z] for x in (0, 0.25, 1) for y in (0, 0.5, 1) for z in (0, 0.75, 1)], F32)
        pts[:len(grid)] = grid
        pts[100:200] = np.abs(pts[100:200]) % 1
        pts[100:150, 0] = 1.0
        pts[150:200, 2] = 0.0
    pts.setflags(write=False)
    return pts


@functools.lru_cache(maxsize=None)
def expected(name, offset):
    return R.ref_mask(region(name), queries(name), offset)


def pack(polys):
    cols = np.ascontiguousarray(np.concatenate([h.T for h in polys], axis=0), F32)
    offs = np.concatenate([[0], np.cumsum([h.shape[1] for h in polys])]).astype(np.uint32)
    return cols, offs


def run_mask(polys, pts, offset, mem="host", dim=3):
    import torch

    from cilantro_amd import capi

    L = capi.load()
    cols, offs = pack(polys)
    n = len(pts)
    if mem == "device":
        t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
        out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = L.cilhip_polytopes_interior_mask(0, cols.ctypes.data, offs.ctypes.data, len(polys), t.data_ptr(), n, dim, capi.MEM_DEVICE, C.c_float(offset), out.data_ptr())
        out = out.cpu().numpy()
    else:
        p = np.ascontiguousarray(pts, F32)
        out = np.full(n, 7, np.uint8)
        rc = L.cilhip_polytopes_interior_mask(0, cols.ctypes.data, offs.ctypes.data, len(polys), p.ctypes.data, n, dim, capi.MEM_HOST, C.c_float(offset), out.ctypes.data)
    assert rc == capi.OK, L.cilhip_last_error(None).decode()
    return out


def run_indices(polys, pts, offset, capacity=None, dim=3):
    from cilantro_amd import capi

    L = capi.load()
    cols, offs = pack(polys)
    p = np.ascontiguousarray(pts, F32)
    n = len(p)
    capacity = n if capacity is None else capacity
    out = np.full(max(capacity, 1), 0xDEADBEEF, np.uint32)
    count = C.c_size_t(12345)
    rc = L.cilhip_polytopes_interior_indices(0, cols.ctypes.data, offs.ctypes.data, len(polys), p.ctypes.data, n, dim, capi.MEM_HOST, C.c_float(offset), out.ctypes.data, capacity,
                                             C.byref(count))
    return rc, count.value, out


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("offset", [0.0, 0.01, -0.01])
@pytest.mark.parametrize("name", ["gauss", "sphere", "cubes", "empty", "everything", "mixed"])
def test_mask_and_indices_equal_the_f32_restatement(name, offset, mem):
    from cilantro_amd import capi

    want = expected(name, offset)
    got = run_mask(region(name), queries(name), offset, mem)
    assert set(np.unique(got)) <= {0, 1}
    assert np.array_equal(got.astype(bool), want)
    if name == "empty":
        assert not want.any()
    if name == "everything":
        assert want.all()
    if name in ("gauss", "cubes") and offset == 0.0:
        assert want.any() and not want.all()
    if mem == "host":
        rc, count, idx = run_indices(region(name), queries(name), offset)
        assert rc == capi.OK and count == int(want.sum())
        assert np.array_equal(idx[:count], np.nonzero(want)[0])
        assert (np.diff(idx[:count].astype(np.int64)) > 0).all()


def test_the_edge_is_exercised():
    """points exactly on the cube's faces are inside at offset 0 (v = 0 is not > -0), outside at 0.01, and the restatement says so"""
    pts = queries("cubes")
    on_face = np.arange(100, 150)
    assert expected("cubes", 0.0)[on_face].all()
    single = R.ref_mask((cube([0, 0, 0]),), pts, 0.01)
    assert not single[on_face].any()
    got = run_mask((cube([0, 0, 0]),), pts, 0.01)
    assert np.array_equal(got.astype(bool), single)


@pytest.mark.parametrize("mem", ["host", "device"])
def test_signed_distances(mem):
    import torch

    from cilantro_amd import capi

    L = capi.load()
    for name, n in (("gauss", 65537), ("sphere", 257)):
        hs = region(name)[0]
        pts = np.ascontiguousarray(queries(name)[:n])
        Fc = hs.shape[1]
        cols = np.ascontiguousarray(hs.T)
        want = R.ref_distances(hs, pts)
        if mem == "device":
            t = torch.from_numpy(pts).cuda()
            out = torch.empty((Fc, n), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            rc = L.cilhip_polytope_signed_distances(0, cols.ctypes.data, Fc, t.data_ptr(), n, 3, capi.MEM_DEVICE, out.data_ptr())
            got = out.cpu().numpy()
        else:
            got = np.empty((Fc, n), F32)
            rc = L.cilhip_polytope_signed_distances(0, cols.ctypes.data, Fc, pts.ctypes.data, n, 3, capi.MEM_HOST, got.ctypes.data)
        assert rc == capi.OK
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_small_sizes(n):
    from cilantro_amd import capi

    for name in ("cubes", "sphere"):
        pts = queries(name)[:n]
        want = R.ref_mask(region(name), pts, 0.0)
        assert np.array_equal(run_mask(region(name), pts, 0.0).astype(bool), want)
        rc, count, idx = run_indices(region(name), pts, 0.0)
        assert rc == capi.OK and np.array_equal(idx[:count], np.nonzero(want)[0])


def test_two_dimensions():
    ref = R.ref_of("gauss2d_65537")
    rng = np.random.default_rng(5)
    pts = (rng.standard_normal((65537, 2)) * 2.5).astype(F32)
    pts[:len(ref["vertices"])] = ref["vertices"]
    polys = (ref["halfspaces"], R.empty_hull(2)["halfspaces"])
    want = R.ref_mask(polys, pts, 0.0)
    assert want.any() and not want.all()
    assert np.array_equal(run_mask(polys, pts, 0.0, dim=2).astype(bool), want)


def test_capacity_rules():
    from cilantro_amd import capi

    want = expected("cubes", 0.0)
    total = int(want.sum())
    rc, count, idx = run_indices(region("cubes"), queries("cubes"), 0.0, capacity=0)
    assert rc == capi.OK and count == total and idx[0] == 0xDEADBEEF
    rc, count, idx = run_indices(region("cubes"), queries("cubes"), 0.0, capacity=total - 1)
    assert rc == capi.ERR_INVALID and count == total and (idx == 0xDEADBEEF).all()
    assert b"capacity" in capi.load().cilhip_last_error(None)
    rc, count, idx = run_indices(region("cubes"), queries("cubes"), 0.0, capacity=total)
    assert rc == capi.OK and np.array_equal(idx[:total], np.nonzero(want)[0])


def test_space_region_mirror():
    import torch

    from cilantro_amd import spatial

    polys = [spatial.ConvexPolytope3f.from_halfspaces(h) for h in region("cubes")]
    reg = spatial.SpaceRegion3f(polys[:1]).unionWith(spatial.SpaceRegion3f(polys[1:]))
    pts = queries("cubes")
    want = expected("cubes", 0.0)
    assert np.array_equal(reg.getInteriorPointsIndexMask(pts), want)
    assert np.array_equal(reg.getInteriorPointIndices(pts), np.nonzero(want)[0])
    t = torch.from_numpy(np.ascontiguousarray(pts)).cuda()
    assert np.array_equal(reg.getInteriorPointsIndexMask(t).cpu().numpy(), want)
    assert np.array_equal(reg.getInteriorPointIndices(t).cpu().numpy().astype(np.int64), np.nonzero(want)[0])
    for i in range(0, 200, 7):
        assert reg.containsPoint(pts[i]) == bool(want[i])
    one = polys[0]
    assert np.array_equal(one.getPointSignedDistancesFromFacets(pts[:500]).view(np.uint32), R.ref_distances(region("cubes")[0], pts[:500]).view(np.uint32))
    # a hull built on the device crops its own cloud: every input point is inside at the band's f32 image
    cloud = R.fixture("gauss65537")
    hull = spatial.ConvexHull3f(cloud, True, True)
    assert np.array_equal(hull.getInteriorPointsIndexMask(cloud, -1e-4), R.ref_mask((R.ref_of("gauss65537")["halfspaces"],), cloud, -1e-4))
    assert hull.getInteriorPointsIndexMask(cloud, -1e-4).all()
