"""The four features that visit "the points within a fixed radius of a query" on the uniform grid -- radius search, connected components,
radius normals, 3-D mean shift -- against ONE neighbour relation stated in numpy, on one small lattice cloud.  They share one piece of
device code (csrc/grid_ball.hpp: the cells a ball can touch and the order its records are visited in), so one wrong bound shows in all
four here.

The relation is the rule of DESIGN.md sections 11 and 13: d2 = ((dx*dx)+(dy*dy))+(dz*dz) in float32, operation by operation, and j is a
neighbour of q iff d2 < radius_sq (strict).  Every coordinate is a multiple of 1/8 below 2^10 in magnitude, so every difference, square
and sum above is exact in float32 and every float64 sum of coordinates is exact: nothing here needs a tolerance, and the order a sum is
taken in cannot show.  The cloud sits off the origin, holds two exact duplicates and two non-finite rows; the queries are points of the
cloud, points beyond each of the six faces of its bounding box (nearer than the radius and farther than it) and one non-finite row; the
radii are 0, one below a grid cell, one about three cells and one larger than the whole box."""
import numpy as np
import pytest

N = 1800
EDGE = 96      # lattice steps of 1/8 per axis: a box of 12 units, about one point per unit volume, grid cells of 1 to 1.3 units
ORIGIN = np.array([100.5, -37.25, 250.125], np.float32)
BEYOND = (0.5, 2.0, 5.0, 64.0)      # how far the outside queries lie beyond a face: on both sides of every positive radius below
RADII = (0.0, 0.75, 3.5, 40.0)      # plain radii; their squares are exact in float32
NONFINITE_ROWS = {411: (np.nan, 3.0, 4.0), 1203: (np.inf, 2.5, -np.inf)}
DUPLICATES = {6: 5, 1500: 78}      # row -> the row it repeats (rows 5 and 78 have no other point within the smallest radius: a pair, not a line of three)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _bits(a):
    return _f32(a).view(np.uint32)


def _d2(q, p):
    """[nq, n] float32, each operation rounded on its own (here: exact)"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = [q[:, None, a] - p[None, :, a] for a in range(3)]
        return ((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])


class Case:
    def __init__(self):
        rng = np.random.default_rng(20261020)
        cells = rng.choice(EDGE ** 3, N, replace=False)      # distinct lattice sites
        ijk = np.stack([cells // (EDGE * EDGE), (cells // EDGE) % EDGE, cells % EDGE], 1)
        p = ORIGIN + _f32(ijk) * np.float32(0.125)
        for row, src in DUPLICATES.items():
            p[row] = p[src]
        for row, xyz in NONFINITE_ROWS.items():
            p[row] = xyz
        self.points = _f32(p)
        self.finite = np.isfinite(p).all(1)
        # queries: 200 points of the cloud (the duplicates and a non-finite row among them), 24 beyond the faces, one non-finite row
        own = np.unique(np.concatenate([rng.choice(N, 195, replace=False), list(DUPLICATES), list(DUPLICATES.values()), [411]]))
        outside = []
        fin = np.nonzero(self.finite)[0]
        for axis in range(3):
            for side, pick in ((-1.0, np.argmin), (1.0, np.argmax)):
                corner = p[fin[pick(p[fin, axis])]]      # a point of the cloud on that face: the outside query is exactly `far` from it
                for far in BEYOND:
                    q = corner.copy()
                    q[axis] += np.float32(side * far)
                    outside.append(q)
        self.queries = _f32(np.concatenate([p[own], outside, [[1.0, np.nan, 2.0]]]))
        self.n_own = len(own)
        assert np.abs(self.points[self.finite]).max() < 1024 and np.abs(self.queries[:-1][np.isfinite(self.queries[:-1]).all(1)]).max() < 1024
        self.d2_queries = _d2(self.queries, self.points)
        self.d2_self = _d2(self.points, self.points)

    def radius_sq(self, r):
        return np.float32(r) * np.float32(r)


@pytest.fixture(scope="module")
def case():
    return Case()


def _components(adj):
    """labels of the connected components of a symmetric boolean matrix: the lowest member of each"""
    n = adj.shape[0]
    lab = np.arange(n)
    while True:
        new = np.minimum(lab, np.where(adj, lab[None, :], n).min(1))
        new = new[new]      # pointer jumping
        if np.array_equal(new, lab):
            return lab
        lab = new


def test_the_cloud_is_what_the_exact_checks_need(case):
    """on the CPU: lattice coordinates, the special rows, outside queries on both sides of every radius, and no neighbourhood of three or
    more points on one line (a normal would not be defined there)"""
    p, q = case.points, case.queries
    fin = case.finite
    assert p.shape == (N, 3) and (~fin).sum() == 2 and not np.isfinite(q[-1]).all()
    assert np.array_equal(p[fin] * 8, np.round(p[fin] * 8)) and np.array_equal(q[:-1][np.isfinite(q[:-1]).all(1)] * 8, np.round(q[:-1][np.isfinite(q[:-1]).all(1)] * 8))
    for row, src in DUPLICATES.items():
        assert np.array_equal(p[row], p[src])
    lo, hi = p[fin].min(0), p[fin].max(0)
    assert np.linalg.norm(hi - lo) < 40.0      # the largest radius holds the whole box
    out = q[case.n_own:-1]
    assert len(out) == 24 and ((out < lo) | (out > hi)).any(1).all()
    nearest = np.sqrt(case.d2_queries[case.n_own:-1][:, fin].min(1).astype(np.float64)).reshape(6, len(BEYOND))
    assert np.array_equal(nearest, np.tile(BEYOND, (6, 1)))      # exactly that far from the cloud
    for r in RADII[1:]:
        assert (nearest < r).any() and (nearest > r).any()
    units = np.round(np.where(fin[:, None], p, 0) * 8).astype(np.int64)
    for r in RADII[1:]:
        inside = case.d2_self < case.radius_sq(r)
        for i in np.nonzero(inside.sum(1) >= 3)[0]:
            v = units[inside[i]] - units[i]
            v = v[(v != 0).any(1)]
            assert len(v) and np.cross(v[0], v).any(), (r, i)


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
def test_radius_search_returns_the_relation_in_order(hip_lib, case, r):
    from cilantro_amd.normal_estimation import KDTree3f

    r2 = case.radius_sq(r)
    off, idx, d2 = KDTree3f(case.points).radiusSearch(case.queries, float(r2))
    inside = case.d2_queries < r2
    assert np.array_equal(np.diff(off), inside.sum(1))
    for qi in range(len(case.queries)):
        want = np.nonzero(inside[qi])[0]
        want = want[np.lexsort((want, case.d2_queries[qi, want]))]      # ascending (d2, index)
        assert np.array_equal(idx[off[qi]:off[qi + 1]], want), qi
        assert np.array_equal(_bits(d2[off[qi]:off[qi + 1]]), _bits(case.d2_queries[qi, want])), qi


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
def test_components_are_the_relations(hip_lib, case, r):
    from cilantro_amd import clustering

    adj = (case.d2_self < case.radius_sq(r)) & ~np.eye(N, dtype=bool)
    root = _components(adj)
    roots, sizes = np.unique(root, return_counts=True)      # (a component's root is its lowest member)
    order = np.lexsort((roots, -sizes))      # size descending, equal sizes by lowest member
    rank = np.empty(N, np.int64)
    rank[roots[order]] = np.arange(len(roots))
    labels = rank[root]
    members = np.argsort(labels, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(sizes[order])])
    got = clustering.connected_components(case.points, float(case.radius_sq(r)))
    for name, g, w in zip(("labels", "offsets", "members"), got, (labels, offsets, members)):
        assert np.array_equal(g, w), name
    assert (sizes[rank[root[~case.finite]]] == 1).all()      # a non-finite point is alone


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
def test_radius_normals_are_finite_where_three_points_are_inside(hip_lib, case, r):
    from cilantro_amd.normal_estimation import NormalEstimation3f

    nrm, curv = NormalEstimation3f(case.points)._run_radius(float(case.radius_sq(r)), True)
    count = (case.d2_self < case.radius_sq(r)).sum(1)      # (the point itself is inside its own ball; a non-finite point is in none)
    assert np.array_equal(np.isfinite(nrm).all(1), count >= 3) and np.array_equal(np.isnan(nrm).all(1), count < 3)
    assert np.array_equal(np.isfinite(curv), count >= 3)


@pytest.mark.gpu
@pytest.mark.parametrize("form", (1, 2))
@pytest.mark.parametrize("r", RADII)
def test_one_mean_shift_pass_is_the_exact_mean(hip_lib, case, r, form):
    from cilantro_amd import clustering

    inside = case.d2_queries < case.radius_sq(r)
    count = inside.sum(1).astype(np.float64)
    p64 = np.where(case.finite[:, None], case.points, 0).astype(np.float64)      # (a non-finite row is in no ball: its term never enters a sum)
    with np.errstate(invalid="ignore"):
        want = ((inside.astype(np.float64) @ p64) / count[:, None]).astype(np.float32)      # every sum exact; 0 / 0 = NaN: an empty ball
    got = clustering.mean_shift(case.points, r, 1, 0.25, seeds=case.queries, form=form)
    assert got["stats"]["form_used"] == form and got["iterations"] == 1
    empty = count == 0
    assert empty[-1] and empty.sum() > 1 and not empty.all() or r == 0.0      # the non-finite seed, and some seed farther out than r
    assert np.array_equal(np.isnan(got["shifted"]).all(1), empty) and np.array_equal(np.isnan(got["shifted"]).any(1), empty)
    assert np.array_equal(_bits(got["shifted"][~empty]), _bits(want[~empty]))
