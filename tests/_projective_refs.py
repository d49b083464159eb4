"""numpy restatements of DESIGN.md section 14 (depth images <-> points), the yardstick of tests/test_gpu_image_conversions.py.

Two forms of every conversion:
  * `*_literal`: a per-pixel / per-point transcription of the reference's loops (core/image_point_cloud_conversions.hpp), run serially,
    with np.float32 scalars so that every product and sum rounds to f32 and nothing is fused;
  * the vectorised form the GPU tests compare against, bit for bit.  tests/test_projective_refs_cpu.py pins the two against each other.

Pinned arithmetic: dot3(a, b) = a0 b0 + (a1 b1 + a2 b2); a point transform is (L_r0 x + (L_r1 y + L_r2 z)) + t_r.  That is what Eigen's
fixed-size products are understood to evaluate; it is unverified against a compiled reference (Eigen is not available to the tests).

Matrices are ordinary numpy matrices here (K[r, c], E[r, c]); the C ABI takes them column-major (`.T.ravel()`)."""
import numpy as np

F = np.float32
U16, F32 = 0, 1
EMPTY = 0xFFFFFFFF
FUSION_K = np.array([[525, 0, 319.5], [0, 525, 239.5], [0, 0, 1]], F)      # examples/fusion.cpp:64
DEFAULT_K = np.array([[528, 0, 320], [0, 528, 240], [0, 0, 1]], F)         # correspondence_search_projective.hpp:33-40


def small_E(angles=(0.04, -0.03, 0.035), t=(0.02, -0.01, 0.03)):
    """a rigid camera pose close to the identity (rotations about x, y, z in radians), f32"""
    cx, cy, cz = np.cos(angles)
    sx, sy, sz = np.sin(angles)
    Rx, Ry, Rz = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]), np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]), np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = Rz @ Ry @ Rx, t
    return E.astype(F)


class Conv:
    """DepthValueConverter / TruncatedDepthValueConverter (:7-51)"""

    def __init__(self, raw_type=U16, scale=1.0, truncated=False, max_depth=np.finfo(F).max):
        self.raw_type, self.scale, self.truncated, self.max_depth = raw_type, F(scale), bool(truncated), F(max_depth)
        self.inv_scale = F(1.0) / self.scale

    @property
    def dtype(self):
        return np.uint16 if self.raw_type == U16 else np.float32


def dot3(a0, a1, a2, b0, b1, b2):
    return a0 * b0 + (a1 * b1 + a2 * b2)


def kinv(K):
    """D2: the inverse of the f32 K formed in f64 (cofactors over the determinant), every entry rounded once"""
    m = np.asarray(K, F).astype(np.float64)
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = m[0, 0] * c00 + m[0, 1] * c01 + m[0, 2] * c02
    inv = np.array([[c00, m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [c01, m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [c02, m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]]) / det
    return inv.astype(F)


def to_cam(E):
    """P1: (R^T, -R^T t) formed in f64 from the f32 entries, rounded once -> (L 3x3, t 3)"""
    e = np.asarray(E, F).astype(np.float64)
    L = e[:3, :3].T
    t = -(L[:, 0] * e[0, 3] + (L[:, 1] * e[1, 3] + L[:, 2] * e[2, 3]))
    return L.astype(F), t.astype(F)


def transform(L, t, p):
    """the pinned point transform on rows of p (n, 3)"""
    L, p = np.asarray(L, F), np.asarray(p, F)
    with np.errstate(all="ignore"):
        cols = [dot3(L[r, 0], L[r, 1], L[r, 2], p[:, 0], p[:, 1], p[:, 2]) + (F(t[r]) if t is not None else F(0)) for r in range(3)]
    return np.stack(cols, axis=1).astype(F)


def linear(L, v):
    L, v = np.asarray(L, F), np.asarray(v, F)
    with np.errstate(all="ignore"):
        return np.stack([dot3(L[r, 0], L[r, 1], L[r, 2], v[:, 0], v[:, 1], v[:, 2]) for r in range(3)], axis=1).astype(F)


def metric(depth, conv):
    """D1"""
    with np.errstate(all="ignore"):
        z = conv.inv_scale * np.asarray(depth).astype(F)
        if conv.truncated:
            z = np.where(z < conv.max_depth, z, F(0))
    return z.astype(F)


def normalized(v):
    """DESIGN section 10 rule 4: v / sqrt(|v|^2) per component if |v|^2 > 0, else v (correctly rounded f32 square root and quotients)"""
    with np.errstate(all="ignore"):
        z = dot3(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2])
        s = np.sqrt(z.astype(F))
        out = np.where((z > 0)[:, None], v / s[:, None], v)
    return out.astype(F)


def camera_points(depth, w, h, K, conv):
    """D1-D3: the camera-frame point of every pixel, (w h, 3)"""
    ki = kinv(K)
    z = metric(np.asarray(depth).reshape(-1), conv)
    k = np.arange(w * h)
    x, y = (k % max(w, 1)).astype(F), (k // max(w, 1)).astype(F)
    with np.errstate(all="ignore"):
        v0, v1 = z * x, z * y
        P = np.stack([dot3(ki[r, 0], ki[r, 1], ki[r, 2], v0, v1, z) for r in range(3)], axis=1)
    return P.astype(F)


def depth_to_points(depth, w, h, K, conv, rgb=None, E=None, keep_invalid=False, want_normals=False):
    """D1-D8 -> (points, normals or None, colours or None)"""
    P = camera_points(depth, w, h, K, conv)
    n = w * h
    N = None
    if want_normals:
        N = np.full((n, 3), np.nan, F)
        if w >= 3 and h >= 3:
            ok = (P[:, 2] > 0).reshape(h, w)
            inner = np.zeros((h, w), bool)
            inner[1:-1, 1:-1] = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
            k = np.flatnonzero(inner.reshape(-1))
            with np.errstate(all="ignore"):
                a, b = P[k + w] - P[k - w], P[k + 1] - P[k - 1]
                c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F)
            N[k] = normalized(c)
        keep = ~np.isnan(N[:, 0])
    else:
        keep = P[:, 2] > 0
    if keep_invalid:
        keep = np.ones(n, bool)
    P = P[keep]
    if N is not None:
        N = N[keep]
    C = None
    if rgb is not None:
        C = ((F(1.0) / F(255.0)) * np.asarray(rgb, np.uint8).reshape(-1, 3).astype(F))[keep].astype(F)
    if E is not None:
        E = np.asarray(E, F)
        P = transform(E[:3, :3], E[:3, 3], P)
        if N is not None:
            N = linear(E[:3, :3], N)
    return P, N, C


def llround(u):
    """ties away from zero, as a float array (u finite)"""
    r = np.trunc(u)
    f = u - r      # exact
    return r + np.where(np.abs(f) >= F(0.5), np.copysign(F(1), u), F(0)).astype(F)


def project(xyz, K, w, h, E=None):
    """P1-P3 -> (indices of the accepted points, their pixels, their camera-frame points)"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    K = np.asarray(K, F)
    c = p if E is None else transform(*to_cam(E), p)
    with np.errstate(all="ignore"):
        ok = c[:, 2] > 0
        inv_z = F(1.0) / c[:, 2]
        u = inv_z * dot3(K[0, 0], K[0, 1], K[0, 2], c[:, 0], c[:, 1], c[:, 2])
        v = inv_z * dot3(K[1, 0], K[1, 1], K[1, 2], c[:, 0], c[:, 1], c[:, 2])
        ok &= np.isfinite(u) & np.isfinite(v)
        x, y = llround(np.where(ok, u, F(0))), llround(np.where(ok, v, F(0)))
        ok &= (x >= 0) & (x < w) & (y >= 0) & (y < h)
    i = np.flatnonzero(ok)
    return i, y[i].astype(np.int64) * w + x[i].astype(np.int64), c[i]


def _winners(i, pix, key):
    """per pixel the entry with the smallest key, then the lowest index -> (pixels, positions into i)"""
    order = np.lexsort((i, key, pix))
    first = np.ones(order.size, bool)
    first[1:] = pix[order][1:] != pix[order][:-1]
    return pix[order][first], order[first]


def points_to_index_map(xyz, K, w, h, E=None):
    """P4 -> uint32 (h w), EMPTY where no point lands"""
    i, pix, c = project(xyz, K, w, h, E)
    out = np.full(w * h, EMPTY, np.uint32)
    px, pos = _winners(i, pix, c[:, 2])
    out[px] = i[pos]
    return out


def raw_values(cz, conv):
    """P5 -> (contributes, raw as float64 for ordering and writing)"""
    with np.errstate(all="ignore"):
        prod = conv.scale * cz
        ok = np.ones(cz.shape, bool)
        if conv.truncated:
            ok &= cz < conv.max_depth
        if conv.raw_type == U16:
            ok &= prod < F(65536)
            raw = np.trunc(np.where(ok, prod, F(0)))
        else:
            raw = prod
        ok &= raw > 0
    return ok, raw


def byte(colour):
    with np.errstate(all="ignore"):
        v = F(255.0) * np.asarray(colour, F)
        v = np.where(v > 0, np.minimum(v, F(255)), F(0))      # NaN -> 0
    return np.trunc(v).astype(np.uint8)


def points_to_depth_image(xyz, K, conv, w, h, E=None, colours=None):
    """P5 -> (depth (h w) of conv.dtype, rgb (h w, 3) uint8 or None)"""
    i, pix, c = project(xyz, K, w, h, E)
    ok, raw = raw_values(c[:, 2], conv)
    i, pix, raw = i[ok], pix[ok], raw[ok]
    depth = np.zeros(w * h, conv.dtype)
    rgb = None if colours is None else np.zeros((w * h, 3), np.uint8)
    px, pos = _winners(i, pix, raw)
    depth[px] = raw[pos].astype(conv.dtype)
    if rgb is not None:
        rgb[px] = byte(np.asarray(colours, F).reshape(-1, 3)[i[pos]])
    return depth, rgb


# ---- the reference's loops, one element at a time ----------------------------------------------------------------------
def _dot_s(a, b):
    return F(a[0] * b[0]) + F(F(a[1] * b[1]) + F(a[2] * b[2]))


def _mul_s(M, v, t=None):
    out = np.array([_dot_s(M[r], v) for r in range(3)], F)
    return out if t is None else (out + np.asarray(t, F)).astype(F)


def depth_to_points_literal(depth, w, h, K, conv, rgb=None, E=None, keep_invalid=False, want_normals=False):
    """:53-695, serially; the keep_invalid branch with extrinsics computes E * (Kinv * v)"""
    ki = kinv(K)
    depth = np.asarray(depth).reshape(-1)
    tmp = np.zeros((w * h, 3), F)
    nrm = np.full((w * h, 3), np.nan, F)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                k = y * w + x
                z = F(conv.inv_scale * F(depth[k]))
                if conv.truncated:
                    z = z if z < conv.max_depth else F(0)
                tmp[k] = _mul_s(ki, np.array([F(z * F(x)), F(z * F(y)), z], F))
        if want_normals:
            for y in range(1, h - 1):
                for x in range(1, w - 1):
                    k = y * w + x
                    if tmp[k, 2] > 0 and tmp[k + 1, 2] > 0 and tmp[k - 1, 2] > 0 and tmp[k + w, 2] > 0 and tmp[k - w, 2] > 0:
                        a, b = tmp[k + w] - tmp[k - w], tmp[k + 1] - tmp[k - 1]
                        c = np.array([F(a[1] * b[2]) - F(a[2] * b[1]), F(a[2] * b[0]) - F(a[0] * b[2]), F(a[0] * b[1]) - F(a[1] * b[0])], F)
                        z = _dot_s(c, c)
                        nrm[k] = c / np.sqrt(z) if z > 0 else c
        P, N, C = [], [], []
        for k in range(w * h):
            if keep_invalid or (not np.isnan(nrm[k, 0]) if want_normals else tmp[k, 2] > 0):
                p, n = tmp[k], nrm[k]
                if E is not None:
                    Ef = np.asarray(E, F)
                    p, n = _mul_s(Ef[:3, :3], p, Ef[:3, 3]), _mul_s(Ef[:3, :3], n)
                P.append(p)
                N.append(n)
                if rgb is not None:
                    C.append([F(F(1.0) / F(255.0)) * F(b) for b in np.asarray(rgb, np.uint8).reshape(-1, 3)[k]])
    arr = lambda rows: np.array(rows, F).reshape(-1, 3)      # noqa: E731
    return arr(P), arr(N) if want_normals else None, arr(C) if rgb is not None else None


def _pixel_literal(c, K, w, h):
    """:883-887 for one camera-frame point -> pixel index or None; llround by Python's decimal-free rule on the exact f32 value"""
    import math

    if not c[2] > 0:
        return None
    inv_z = F(1.0) / c[2]
    u, v = F(inv_z * _dot_s(K[0], c)), F(inv_z * _dot_s(K[1], c))
    if not (math.isfinite(u) and math.isfinite(v)):
        return None
    xy = []
    for val in (float(u), float(v)):      # (a double holds an f32 exactly)
        r = math.floor(abs(val) + 0.5)    # |val| + 0.5 is exact in f64 for every f32 that has a fraction
        xy.append(int(math.copysign(r, val)))
    x, y = xy
    if x < 0 or y < 0 or x >= w or y >= h:
        return None
    return y * w + x


def points_to_index_map_literal(xyz, K, w, h, E=None):
    """:865-934, the loop run serially"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    K = np.asarray(K, F)
    cam = to_cam(E) if E is not None else None
    out = np.full(w * h, EMPTY, np.uint32)
    cz = {}
    with np.errstate(all="ignore"):
        for i in range(p.shape[0]):
            c = p[i] if cam is None else _mul_s(cam[0], p[i], cam[1])
            ind = _pixel_literal(c, K, w, h)
            if ind is None:
                continue
            if out[ind] == EMPTY or c[2] < cz[ind]:
                out[ind], cz[ind] = i, c[2]
    return out


def points_to_depth_image_literal(xyz, K, conv, w, h, E=None, colours=None):
    """:697-863, the loop run serially"""
    p = np.asarray(xyz, F).reshape(-1, 3)
    K = np.asarray(K, F)
    cam = to_cam(E) if E is not None else None
    depth = np.zeros(w * h, conv.dtype)
    rgb = None if colours is None else np.zeros((w * h, 3), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(p.shape[0]):
            c = p[i] if cam is None else _mul_s(cam[0], p[i], cam[1])
            ind = _pixel_literal(c, K, w, h)
            if ind is None:
                continue
            if conv.truncated and not c[2] < conv.max_depth:
                continue
            prod = F(conv.scale * c[2])
            if conv.raw_type == U16:
                if not prod < 65536:
                    continue
                val = np.uint16(int(prod))
            else:
                val = prod
            if val > 0 and (depth[ind] == 0 or val < depth[ind]):
                depth[ind] = val
                if rgb is not None:
                    rgb[ind] = byte(np.asarray(colours, F).reshape(-1, 3)[i])
    return depth, rgb


# ---- a synthetic ray-cast scene: a plane and a sphere in front of it, in millimetres ------------------------------------
def raycast_scene(w=67, h=45, K=None):
    """-> (uint16 depth image (h, w), K): z of the nearer of the plane z = 2 m and a sphere of radius 0.4 m at (0.1, -0.05, 1.5), computed
    in f64 per pixel ray and rounded to whole millimetres"""
    K = np.array([[60.0, 0, (w - 1) / 2], [0, 60.0, (h - 1) / 2], [0, 0, 1]], F) if K is None else K
    ys, xs = np.mgrid[0:h, 0:w]
    d = np.stack([(xs - float(K[0, 2])) / float(K[0, 0]), (ys - float(K[1, 2])) / float(K[1, 1]), np.ones((h, w))], axis=-1)      # z = 1 rays
    z = np.full((h, w), 2.0)
    ctr, rad = np.array([0.1, -0.05, 1.5]), 0.4
    a, b, c = (d * d).sum(-1), -2 * (d @ ctr), ctr @ ctr - rad * rad
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = (-b - np.sqrt(np.where(hit, disc, 0))) / (2 * a)
    z = np.where(hit & (t > 0), t, z)
    return np.rint(z * 1000).astype(np.uint16), K


# ---- projective association (rules S1-S3) --------------------------------------------------------
def projective_search(dst, src, T, max_sq_dist, K=None, w=640, h=480, E=None):
    """-> (nn_idx uint32 per source point, EMPTY where none; value f32).  S1: the target's index map under E; S2: q = T s by the
    engine's pinned transform, projected like a map point, value = dx^2 + (dy^2 + dz^2), kept iff value < max_sq_dist (strict)"""
    K = DEFAULT_K if K is None else np.asarray(K, F)
    dst, src, T = np.asarray(dst, F).reshape(-1, 3), np.asarray(src, F).reshape(-1, 3), np.asarray(T, F)
    index = points_to_index_map(dst, K, w, h, E)
    q = transform(T[:3, :3], T[:3, 3], src)
    i, pix, _ = project(q, K, w, h, E)
    nn = np.full(src.shape[0], EMPTY, np.uint32)
    val = np.zeros(src.shape[0], F)
    j = index[pix]
    hit = j != EMPTY
    i, j = i[hit], j[hit]
    with np.errstate(all="ignore"):
        d = q[i] - dst[j]
        v = d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        keep = v < F(max_sq_dist)
    nn[i[keep]], val[i[keep]] = j[keep], v[keep]
    return nn, val


def projective_search_literal(dst, src, T, max_sq_dist, K=None, w=640, h=480, E=None):
    """correspondence_search_projective.hpp:156-209 one source point at a time, over the serial index map"""
    K = DEFAULT_K if K is None else np.asarray(K, F)
    dst, src, T = np.asarray(dst, F).reshape(-1, 3), np.asarray(src, F).reshape(-1, 3), np.asarray(T, F)
    index = points_to_index_map_literal(dst, K, w, h, E)
    cam = to_cam(E) if E is not None else None
    nn = np.full(src.shape[0], EMPTY, np.uint32)
    val = np.zeros(src.shape[0], F)
    with np.errstate(all="ignore"):
        for i in range(src.shape[0]):
            q = _mul_s(T[:3, :3], src[i], T[:3, 3])
            c = q if cam is None else _mul_s(cam[0], q, cam[1])
            ind = _pixel_literal(c, K, w, h)
            if ind is None or index[ind] == EMPTY:
                continue
            d = q - dst[index[ind]]
            v = F(d[0] * d[0]) + F(F(d[1] * d[1]) + F(d[2] * d[2]))
            if v < F(max_sq_dist):
                nn[i], val[i] = index[ind], v
    return nn, val


# ---- crafted scenes for the projective search (tests/test_gpu_projective_edges.py; pinned on the CPU in test_projective_refs_cpu.py) ----
TIE_K = np.array([[4, 0, 3.5], [0, 4, 2.5], [0, 0, 1]], F)       # every entry dyadic: with z a power of two u and v are exact in f32
EDGE_K = np.array([[4, 0, 0], [0, 4, 0], [0, 0, 1]], F)          # the principal point at pixel (0, 0): u = 4 x / z with no sum at all


def tie_scene(w=8, h=6, G=64, seed=0, K=TIE_K):
    """-> (points (w h (G + 1), 3), group (same length): the pixel whose minimal-depth group the point belongs to, -1 for the far points).
    Per pixel G points at ONE depth (1 or 2, alternating with (x + y) % 2) on a 1/64-pixel lattice strictly inside the pixel's footprint
    (|du|, |dv| <= 31/64; the two opposite corners always among them, so every group spans 62/64 of the footprint on both axes), and one
    farther point at z = 4 on the centre ray, which must lose; one random permutation over the whole array, so that the index order has
    nothing to do with where a point lies.  All arithmetic is exact: u, v are multiples of 1/64, (u - cx) z / fx of 1/256."""
    rng = np.random.default_rng(seed)
    K = np.asarray(K, F)
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    pts, grp = [], []
    for y in range(h):
        for x in range(w):
            z = 1.0 if (x + y) % 2 == 0 else 2.0
            sites = np.concatenate([[0, 63 * 63 - 1], 1 + rng.choice(63 * 63 - 2, G - 2, replace=False)])      # (the two corners first)
            du, dv = (sites % 63 - 31) / 64.0, (sites // 63 - 31) / 64.0
            pts.append(np.stack([(x + du - cx) / fx * z, (y + dv - cy) / fy * z, np.full(G, z)], axis=1))
            pts.append(np.array([[(x - cx) / fx * 4.0, (y - cy) / fy * 4.0, 4.0]]))
            grp += [y * w + x] * G + [-1]
    pts, grp = np.concatenate(pts), np.array(grp, np.int64)
    assert np.array_equal(pts.astype(F).astype(np.float64), pts)
    perm = rng.permutation(pts.shape[0])
    return pts[perm].astype(F), grp[perm]


def computed_uv(xyz, K):
    """P2 for camera-frame points, by project()'s arithmetic -> (u, v) f32"""
    c, K = np.asarray(xyz, F).reshape(-1, 3), np.asarray(K, F)
    with np.errstate(all="ignore"):
        inv_z = F(1.0) / c[:, 2]
        return (inv_z * dot3(K[0, 0], K[0, 1], K[0, 2], c[:, 0], c[:, 1], c[:, 2]), inv_z * dot3(K[1, 0], K[1, 1], K[1, 2], c[:, 0], c[:, 1], c[:, 2]))


def _coordinate_for(want, axis, other, z, K):
    """the f32 coordinate on `axis` (0: x, 1: y) at depth z whose COMPUTED projection is exactly `want`, the other axis fixed at `other`;
    searched among the neighbours of the generating formula's value, None if none of them gives it"""
    K = np.asarray(K, F)
    x = F((float(want) - float(K[axis, 2])) / float(K[axis, axis]) * float(z))
    cands = [x]
    lo = hi = x
    for _ in range(64):
        lo, hi = np.nextafter(lo, F(-np.inf)), np.nextafter(hi, F(np.inf))
        cands += [lo, hi]
    for cnd in cands:
        p = np.array([[cnd, other, z]] if axis == 0 else [[other, cnd, z]], F)
        if computed_uv(p, K)[axis][0] == F(want) and np.signbit(computed_uv(p, K)[axis][0]) == np.signbit(F(want)):
            return cnd
    return None


def boundary_values(n):
    """the projections rule P3 decides at the edges of an axis of n pixels"""
    return [F(-0.5), np.nextafter(F(-0.5), F(0)), F(-0.25), F(0.5), F(1.5), F(2.5), F(n - 1), np.nextafter(F(n - 0.5), F(0)), F(n - 0.5)]


def llround_exact(u):
    """llround of one finite f32 by integer arithmetic on its exact value (ties away from zero)"""
    from fractions import Fraction as Q

    q = abs(Q(float(u))) + Q(1, 2)
    r = q.numerator // q.denominator
    return -r if float(u) < 0 else r


def boundary_points(w, h, K=EDGE_K):
    """-> (points, pixel): points of depth 1, 2 and 0.5 whose COMPUTED u (then v) is exactly each of boundary_values(), the other axis on
    the centre of an inner pixel; then points the rules must reject whatever their ray: c_z of +0, -0, the smallest denormal, a negative
    number, NaN, +inf; |u| or |v| at 2^31, the largest f32 below 2^32, 2^32, 2^40, +-inf out of a finite x; a NaN x, a NaN y, an infinite x.
    pixel: what rule P3 gives each (llround by integer arithmetic, -1: rejected), not what project() says.

    K: the sum fx x + cx z must not cancel -- with cx = 3.5, fx = 4 and u near -0.5 it is a multiple of 2^-22, and the float just above
    -0.5 (2^-25 away) is no computed u of any point -- hence EDGE_K, whose u = 4 x / z reaches every f32."""
    K = np.asarray(K, F)
    pts, pix = [], []
    col, row = min(3, w - 1), min(2, h - 1)      # the pixel the other axis stays on
    for z in (1.0, 2.0, 0.5):
        other_x, other_y = _coordinate_for(F(col), 0, F(0), z, K), _coordinate_for(F(row), 1, F(0), z, K)
        for axis, n, other in ((0, w, other_y), (1, h, other_x)):
            for want in boundary_values(n):
                cnd = _coordinate_for(want, axis, other, z, K)
                if cnd is None:
                    raise ValueError(f"no point at depth {z} projects onto {want!r} on axis {axis} under this K")
                pts.append([cnd, other, z] if axis == 0 else [other, cnd, z])
                r = llround_exact(want)
                pix.append(-1 if not 0 <= r < n else (row * w + r if axis == 0 else r * w + col))
    x0, y0 = _coordinate_for(F(col), 0, F(0), 1.0, K), _coordinate_for(F(row), 1, F(0), 1.0, K)
    for cz in (0.0, -0.0, np.finfo(F).smallest_subnormal, -1.0, np.nan, np.inf):
        pts.append([x0, y0, cz])
        pix.append(-1)
    fx = float(K[0, 0])
    big = [2.0 ** 31 / fx, (2.0 ** 32 - 256) / fx, 2.0 ** 32 / fx, 2.0 ** 40 / fx, 3e38, -(2.0 ** 32) / fx, -3e38, np.nan, np.inf, -np.inf]
    for b in big:
        pts += [[b, y0, 1.0], [x0, b, 1.0]]
        pix += [-1, -1]
    return np.array(pts, F), np.array(pix, np.int64)


def organized_scene(offset=(1.0 / 1024, -1.0 / 2048, 1.0 / 1024)):
    """the 67 x 45 ray-cast scene unprojected with normals: one target point per inner pixel; the source is every third target point moved
    by a fixed dyadic offset -> (target, normals, source, K, w, h)"""
    depth, K = raycast_scene()
    w, h = 67, 45
    P, N, _ = depth_to_points(depth, w, h, K, Conv(U16, 1000.0), want_normals=True)
    src = (P[::3] + np.array(offset, F)).astype(F)
    return P, N, src, K, w, h
