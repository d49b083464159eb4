"""The yardstick of DESIGN.md section 20: convex hulls from scipy.spatial.ConvexHull (Qhull) on the f64 image of the f32 input, put into
the project's canonical order, plus the f32 containment expressions in numpy.  Nothing here calls the library under test.

    fixture(name)                 the seeded inputs (float32, n x dim)
    tol_of(points, merge_tol)     the band
    ref_hull(points, simplicial)  dict: is_empty, vertex_point_indices, vertices, facets, facet_neighbors, vertex_facets, planes (f64),
                                  halfspaces (f32, (dim + 1) x F), interior_point, area, volume
    ref_distances / ref_mask      ((h0 x + h1 y) + h2 z) + h3 in f32, left to right
"""
import functools

import numpy as np

F32 = np.float32


# ---- inputs ---------------------------------------------------------------------------------------------------------
DEMO9 = [[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 0.5]]


def _sphere(n, seed):
    g = np.random.default_rng(seed).standard_normal((n, 3))
    return (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    rng = np.random.default_rng(abs(hash_name(name)))
    if name == "tetra4":
        a = rng.uniform(-1, 1, (4, 3))
    elif name == "demo9":
        a = np.array(DEMO9)
    elif name == "cube12":
        a = np.array(DEMO9 + [[0.5, 0.5, 0], [0.5, 0, 0], [1, 1, 1]])
    elif name == "unit257":
        a = rng.uniform(0, 1, (257, 3))
    elif name == "gauss65537" or name == "big":
        a = rng.standard_normal((65537, 3))
    elif name == "offset_aniso65537":
        a = rng.standard_normal((65537, 3)) * np.array([1, 0.2, 0.05]) + np.array([1000.0, -2000.0, 500.0])
    elif name == "sphere3000":
        a = _sphere(3000, 7)
    elif name == "shell_solid23000":
        inner = rng.standard_normal((20000, 3))
        inner = inner / np.linalg.norm(inner, axis=1, keepdims=True) * rng.uniform(0, 0.9, (20000, 1))
        a = np.concatenate([_sphere(3000, 7), inner])
    elif name == "gauss2d_65537":
        a = rng.standard_normal((65537, 2))
    elif name == "square9":      # the corners, the edge midpoints, the centre
        a = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0], [1, 0.5], [0.5, 1], [0, 0.5], [0.5, 0.5]])
    elif name == "nonfinite":
        a = fixture("unit257").astype(np.float64)
        a = np.insert(a, [0, 5, 5, 100, 256, 257], [[np.nan, 0, 0], [np.inf, 0.5, 0.5], [0.5, -np.inf, 0.5], [0.2, 0.2, np.nan], [np.inf, np.inf, np.inf], [0.1, 0.1, -np.inf]], axis=0)
    elif name == "three_points":
        a = rng.uniform(-1, 1, (3, 3))
    elif name == "collinear300":      # integer multiples of a dyadic step: exact in f32
        a = rng.integers(-500, 500, (300, 1)) * np.array([[1.0, 2.0, -1.0]]) / 1024.0
    elif name == "coplanar300":       # on x + y - 2 z = 0, exactly
        xy = rng.integers(0, 1024, (300, 2)) / 1024.0
        a = np.concatenate([xy, (xy[:, :1] + xy[:, 1:]) / 2.0], axis=1)
    elif name == "copies300":
        a = np.tile(np.array([[0.25, -1.5, 3.0]]), (300, 1))
    elif name == "flat_noisy300":     # coplanar300 with noise of 1e-3 off the plane
        a = fixture("coplanar300").astype(np.float64) + rng.uniform(-1e-3, 1e-3, (300, 1)) * np.array([[1.0, 1.0, -2.0]]) / np.sqrt(6.0)
    else:
        raise KeyError(name)
    a = np.ascontiguousarray(a, F32)
    a.setflags(write=False)
    return a


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


GENERAL_3D = ["tetra4", "unit257", "gauss65537", "offset_aniso65537", "sphere3000"]
ALL_3D = ["tetra4", "demo9", "cube12", "unit257", "gauss65537", "offset_aniso65537", "sphere3000", "shell_solid23000", "nonfinite"]
ALL_2D = ["gauss2d_65537", "square9"]
DEGENERATE = ["three_points", "collinear300", "coplanar300", "copies300"]


# ---- the band and the planes ----------------------------------------------------------------------------------------
def tol_of(points, merge_tol=0.0):
    a = np.abs(np.asarray(points, np.float64))
    a = a[np.isfinite(a)]
    m = float(a.max()) if a.size else 0.0
    return max(float(merge_tol), m * 2.0 ** -44)


def plane3(a, b, c):
    """floats in, (nx, ny, nz, off) out; every operation written out (Python floats: IEEE f64, no contraction)"""
    u0, u1, u2 = b[0] - a[0], b[1] - a[1], b[2] - a[2]
    v0, v1, v2 = c[0] - a[0], c[1] - a[1], c[2] - a[2]
    x, y, z = u1 * v2 - u2 * v1, u2 * v0 - u0 * v2, u0 * v1 - u1 * v0
    ln = float(np.sqrt((x * x + y * y) + z * z))
    x, y, z = x / ln, y / ln, z / ln
    return (x, y, z, -((x * a[0] + y * a[1]) + z * a[2]))


def plane2(a, b):
    x, y = b[1] - a[1], -(b[0] - a[0])
    ln = float(np.sqrt(x * x + y * y))
    x, y = x / ln, y / ln
    return (x, y, -(x * a[0] + y * a[1]))


def dist_all(planes, pts):
    """f64 d of every point from every plane, (F, n); the decision expression, left to right"""
    planes = np.asarray(planes, np.float64)
    pts = np.asarray(pts, np.float64)
    d = planes[:, :1] * pts[None, :, 0] + planes[:, 1:2] * pts[None, :, 1]
    if pts.shape[1] == 3:
        d = d + planes[:, 2:3] * pts[None, :, 2]
    return d + planes[:, -1:]


def empty_hull(dim, n_nonfinite=0):
    hs = np.zeros((dim + 1, 2), F32)
    hs[0, 0], hs[dim, 0], hs[0, 1], hs[dim, 1] = 1, 1, -1, 1
    return dict(dim=dim, is_empty=True, vertex_point_indices=np.zeros(0, np.uint32), vertices=np.zeros((0, dim), F32), facets=[], facet_neighbors=[], vertex_facets=[],
                planes=np.zeros((0, dim + 1)), halfspaces=hs, interior_point=np.full(dim, np.nan, F32), area=0.0, volume=0.0, n_nonfinite=n_nonfinite)


def _merge_triangles(P, tris, tol):
    """oriented triangles (input indices) -> boundary polygons of the groups of coplanar neighbours, vertices of degree 2 removed"""
    T = len(tris)
    owner = {}
    for t, tr in enumerate(tris):
        for j in range(3):
            owner[(tr[j], tr[(j + 1) % 3])] = (t, j)
    pl = [plane3(P[tr[0]], P[tr[1]], P[tr[2]]) for tr in tris]
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def d(h, p):
        return ((h[0] * p[0] + h[1] * p[1]) + h[2] * p[2]) + h[3]

    for t, tr in enumerate(tris):
        for j in range(3):
            u, ju = owner[(tr[(j + 1) % 3], tr[j])]
            if u <= t:
                continue
            if abs(d(pl[u], P[tr[(j + 2) % 3]])) <= tol and abs(d(pl[t], P[tris[u][(ju + 2) % 3]])) <= tol:
                a, b = find(t), find(u)
                if a != b:
                    parent[max(a, b)] = min(a, b)
    nxt = {}
    for t, tr in enumerate(tris):
        g = find(t)
        for j in range(3):
            a, b = tr[j], tr[(j + 1) % 3]
            if find(owner[(b, a)][0]) != g:
                assert a not in nxt.setdefault(g, {})
                nxt[g][a] = b
    polys = []
    for g in sorted(nxt):
        m = nxt[g]
        start = min(m)
        p, v = [start], m[start]
        while v != start:
            p.append(v)
            v = m[v]
        assert len(p) == len(m)
        polys.append(p)
    deg = {}
    for p in polys:
        for v in p:
            deg[v] = deg.get(v, 0) + 1
    return [[v for v in p if deg[v] >= 3] for p in polys]


def ref_hull(points, simplicial=True, merge_tol=0.0):
    from scipy.spatial import ConvexHull
    from scipy.spatial import QhullError

    pts32 = np.asarray(points, F32)
    dim = pts32.shape[1] if pts32.ndim == 2 else 3
    finite = np.isfinite(pts32).all(axis=1) if len(pts32) else np.zeros(0, bool)
    n_nonfinite = int((~finite).sum())
    keep = np.nonzero(finite)[0]
    if len(keep) < dim + 1:
        return empty_hull(dim, n_nonfinite)
    P64 = pts32[keep].astype(np.float64)
    tol = tol_of(P64, merge_tol)
    try:
        hull = ConvexHull(P64)
    except QhullError:
        return empty_hull(dim, n_nonfinite)
    # of exact duplicates the lowest index is the vertex
    used = np.unique(hull.simplices)
    remap = {}
    if len(used):
        first_of = {}
        for i in range(len(P64)):
            key = P64[i].tobytes()
            if key not in first_of:
                first_of[key] = i
        remap = {int(v): first_of[P64[v].tobytes()] for v in used}
    Pl = [tuple(float(c) for c in row) for row in P64]
    if dim == 3:
        tris = []
        for s, eq in zip(hull.simplices, hull.equations):
            a, b, c = (remap[int(v)] for v in s)
            h = plane3(Pl[a], Pl[b], Pl[c])
            if h[0] * eq[0] + h[1] * eq[1] + h[2] * eq[2] < 0:
                b, c = c, b
            tris.append((a, b, c))
        polys = _merge_triangles(Pl, tris, tol)
        vs = sorted({v for p in polys for v in p})
        loc = {v: k for k, v in enumerate(vs)}
        facets = []
        for p in polys:
            q = [loc[v] for v in p]
            k = q.index(min(q))
            q = q[k:] + q[:k]
            if simplicial:
                facets += [[q[0], q[i], q[i + 1]] for i in range(1, len(q) - 1)]
            else:
                facets.append(q)
        facets.sort()
    else:
        edges = []
        for s, eq in zip(hull.simplices, hull.equations):
            a, b = (remap[int(v)] for v in s)
            h = plane2(Pl[a], Pl[b])
            if h[0] * eq[0] + h[1] * eq[1] < 0:
                a, b = b, a
            edges.append((a, b))
        vs = sorted({v for e in edges for v in e})
        loc = {v: k for k, v in enumerate(vs)}
        facets = sorted([loc[a], loc[b]] for a, b in edges)
    V = len(vs)
    verts32 = pts32[keep][vs]
    acc = np.zeros(dim, F32)
    for row in verts32:
        acc = (acc + row).astype(F32)
    interior = (acc / F32(V)).astype(F32)
    c0 = [float(x) for x in interior]
    vp = [Pl[v] for v in vs]
    planes, area, volume = [], 0.0, 0.0
    owner = {}
    for k, f in enumerate(facets):
        if dim == 3:
            best = min(range(1, len(f) - 1), key=lambda i: (min(f[i], f[i + 1]), max(f[i], f[i + 1])))
            planes.append(plane3(vp[f[0]], vp[f[best]], vp[f[best + 1]]))
            for i in range(1, len(f) - 1):
                a, b, c = vp[f[0]], vp[f[i]], vp[f[i + 1]]
                u = [b[j] - a[j] for j in range(3)]
                v = [c[j] - a[j] for j in range(3)]
                x, y, z = u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]
                area += 0.5 * float(np.sqrt((x * x + y * y) + z * z))
                A = [a[j] - c0[j] for j in range(3)]
                B = [b[j] - c0[j] for j in range(3)]
                Cc = [c[j] - c0[j] for j in range(3)]
                bx, by, bz = B[1] * Cc[2] - B[2] * Cc[1], B[2] * Cc[0] - B[0] * Cc[2], B[0] * Cc[1] - B[1] * Cc[0]
                volume += ((A[0] * bx + A[1] * by) + A[2] * bz) / 6.0
            for j in range(len(f)):
                owner[(f[j], f[(j + 1) % len(f)])] = k
        else:
            p, q = vp[f[0]], vp[f[1]]
            planes.append(plane2(p, q))
            area += float(np.sqrt((q[0] - p[0]) ** 2 + (q[1] - p[1]) ** 2))
            volume += 0.5 * ((p[0] - c0[0]) * (q[1] - c0[1]) - (p[1] - c0[1]) * (q[0] - c0[0]))
    if dim == 3:
        nbrs = [[owner[(f[(j + 1) % len(f)], f[j])] for j in range(len(f))] for f in facets]
    else:
        starts = {f[0]: k for k, f in enumerate(facets)}
        ends = {f[1]: k for k, f in enumerate(facets)}
        nbrs = [[ends[f[0]], starts[f[1]]] for f in facets]
    vf = [[] for _ in range(V)]
    for k, f in enumerate(facets):
        for v in f:
            vf[v].append(k)
    planes = np.array(planes, np.float64).reshape(len(facets), dim + 1)
    return dict(dim=dim, is_empty=False, vertex_point_indices=keep[vs].astype(np.uint32), vertices=verts32, facets=facets, facet_neighbors=nbrs, vertex_facets=[sorted(x) for x in vf],
                planes=planes, halfspaces=np.ascontiguousarray(planes.T.astype(F32)), interior_point=interior, area=area, volume=volume, n_nonfinite=n_nonfinite,
                scipy_area=float(hull.area), scipy_volume=float(hull.volume), tol=tol)


@functools.lru_cache(maxsize=None)
def ref_of(name, simplicial=True):
    return ref_hull(fixture(name), simplicial)


def sum_bounds(points, n_facets):
    """the rounding bounds of the issue: F 64 2^-53 M R^2 for the volume, F 64 2^-53 M R for the area"""
    a = np.asarray(points, np.float64)
    a = a[np.isfinite(a).all(axis=1)]
    M = float(np.abs(a).max())
    R = float(np.linalg.norm(a.max(axis=0) - a.min(axis=0)))
    return n_facets * 64 * 2.0 ** -53 * M * R * R, n_facets * 64 * 2.0 ** -53 * M * R


# ---- containment ----------------------------------------------------------------------------------------------------
def ref_distances(halfspaces, pts):
    """halfspaces (dim + 1, F) f32, pts (n, dim) f32 -> (F, n) f32: ((h0 x + h1 y) + h2 z) + h3"""
    h = np.asarray(halfspaces, F32)
    p = np.asarray(pts, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = (h[0][:, None] * p[None, :, 0]).astype(F32) + (h[1][:, None] * p[None, :, 1]).astype(F32)
        if p.shape[1] == 3:
            v = v.astype(F32) + (h[2][:, None] * p[None, :, 2]).astype(F32)
        return (v.astype(F32) + h[-1][:, None]).astype(F32)


def ref_mask(polys, pts, offset):
    """polys: list of (dim + 1, F_p) f32 arrays.  Inside a polytope iff no facet value > -offset; inside the region iff inside any."""
    pts = np.asarray(pts, F32)
    inside = np.zeros(len(pts), bool)
    lim = -F32(offset)
    for h in polys:
        if h.shape[1] == 0:
            inside[:] = True
            continue
        ok = np.ones(len(pts), bool)
        for c0 in range(0, h.shape[1], 512):
            with np.errstate(invalid="ignore"):
                ok &= ~(ref_distances(h[:, c0:c0 + 512], pts) > lim).any(axis=0)
        inside |= ok
    return inside
