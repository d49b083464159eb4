"""CPU: the yardstick of the image conversions is sound.  tests/_projective_refs.py holds a literal, one-element-at-a-time transcription
of the reference's loops (core/image_point_cloud_conversions.hpp) and the vectorised restatement the GPU tests compare against; here
the two are pinned against each other on small inputs, and the facts DESIGN.md section 14 quotes about tests/golden/frames_full.npz
are asserted."""
import os

import numpy as np
import pytest

import _projective_refs as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frames_full.npz")
E_SMALL = R.small_E()


def same(a, b):
    """bit-equal, NaN matching NaN"""
    if a is None or b is None:
        return a is None and b is None
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


@pytest.fixture(scope="module")
def p1():
    return np.load(GOLDEN)["p1"]


def small_depth(w, h, seed, raw_type):
    rng = np.random.default_rng(seed)
    d = rng.integers(400, 3000, size=(h, w)).astype(np.uint16)
    d[rng.random((h, w)) < 0.2] = 0
    if raw_type == R.F32:
        d = d.astype(F)
        d.reshape(-1)[:: 7] = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0], F)[np.arange(d.reshape(-1)[:: 7].size) % 5]
    return d


@pytest.mark.parametrize("w,h", [(1, 1), (2, 5), (5, 2), (3, 3), (9, 7)])
@pytest.mark.parametrize("raw_type", [R.U16, R.F32])
@pytest.mark.parametrize("keep_invalid,want_normals,with_e", [(0, 0, 0), (0, 1, 0), (1, 1, 1), (1, 0, 1), (0, 1, 1)])
def test_depth_to_points_restatement_is_the_literal_loop(w, h, raw_type, keep_invalid, want_normals, with_e):
    depth = small_depth(w, h, w * 31 + h, raw_type)
    rgb = np.random.default_rng(5).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    conv = R.Conv(raw_type, 1000.0, truncated=True, max_depth=2.5)
    K = np.array([[12.5, 0, (w - 1) / 2], [0, 12.25, (h - 1) / 2], [0, 0, 1]], F)
    args = dict(rgb=rgb, E=E_SMALL if with_e else None, keep_invalid=bool(keep_invalid), want_normals=bool(want_normals))
    got, lit = R.depth_to_points(depth, w, h, K, conv, **args), R.depth_to_points_literal(depth, w, h, K, conv, **args)
    for g, l in zip(got, lit):
        assert same(g, l)
    if keep_invalid:
        assert got[0].shape[0] == w * h
    if want_normals and (w < 3 or h < 3) and not keep_invalid:
        assert got[0].shape[0] == 0      # no interior pixel: no normals exist


def splat_cloud(seed, n=300):
    """points in front of, behind and beside a 9 x 7 camera, with ties in z and several per pixel"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-0.6, 0.6, n), rng.uniform(-0.5, 0.5, n), rng.choice([0.5, 0.75, 1.0, 1.5, -1.0, 0.0], n)], axis=1).astype(F)
    p[::17] = np.array([np.nan, 0.1, 1.0], F)
    p[5::23, 2] = np.inf
    return p


@pytest.mark.parametrize("with_e", [0, 1])
def test_index_map_restatement_is_the_serial_loop(with_e):
    p, K = splat_cloud(1), np.array([[6.0, 0, 4.0], [0, 6.0, 3.0], [0, 0, 1]], F)
    E = E_SMALL if with_e else None
    got = R.points_to_index_map(p, K, 9, 7, E)
    assert np.array_equal(got, R.points_to_index_map_literal(p, K, 9, 7, E))
    assert (got != R.EMPTY).sum() > 20


@pytest.mark.parametrize("conv", [R.Conv(R.U16, 1000.0), R.Conv(R.U16, 1000.0, True, 1.0), R.Conv(R.F32, 2.0), R.Conv(R.U16, 70000.0)], ids=["u16", "u16-trunc", "f32", "u16-overflow"])
@pytest.mark.parametrize("with_e", [0, 1])
def test_depth_image_restatement_is_the_serial_loop(conv, with_e):
    p, K = splat_cloud(2), np.array([[6.0, 0, 4.0], [0, 6.0, 3.0], [0, 0, 1]], F)
    col = np.random.default_rng(3).uniform(-0.2, 1.3, p.shape).astype(F)
    col[::11] = np.nan
    E = E_SMALL if with_e else None
    got, lit = R.points_to_depth_image(p, K, conv, 9, 7, E, col), R.points_to_depth_image_literal(p, K, conv, 9, 7, E, col)
    assert same(got[0], lit[0]) and np.array_equal(got[1], lit[1])


def test_pixel_rounding_is_llround_not_rint():
    """P3 by construction: K = identity-like, z = 1, so u = x"""
    K = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], F)
    w = 4
    us = np.array([-0.4, -0.5, 0.5, 1.5, 2.5, w - 0.5, w - 0.75, np.nextafter(F(0.5), F(0))], F)
    p = np.stack([us, np.zeros_like(us), np.ones_like(us)], axis=1)
    i, pix, _ = R.project(p, K, w, 1)
    assert dict(zip(i.tolist(), pix.tolist())) == {0: 0, 2: 1, 3: 2, 4: 3, 6: 3, 7: 0}      # -0.5 -> -1 and w - 0.5 -> w are outside
    assert np.array_equal(R.points_to_index_map(p, K, w, 1), R.points_to_index_map_literal(p, K, w, 1))
    assert np.array_equal(R.byte(np.array([-0.1, 0.0, 0.5, 1.0, 1.2, np.nan, np.inf], F)), np.array([0, 0, 127, 255, 255, 0, 255], np.uint8))


def test_frames_full_under_the_fusion_camera(p1):
    """tests/golden/frames_full.npz is an unprojected 640 x 480 millimetre frame (K of examples/fusion.cpp:64)"""
    conv = R.Conv(R.U16, 1000.0)
    i, pix, c = R.project(p1, R.FUSION_K, 640, 480)
    assert i.size == p1.shape[0] == 120111 and np.unique(pix).size == 118703
    assert (np.unique(pix, return_counts=True)[1] > 1).sum() == 1400
    depth, _ = R.points_to_depth_image(p1, R.FUSION_K, conv, 640, 480)
    assert np.count_nonzero(depth) == 118703
    # points that lose their pixel to a point of bit-equal z: the winner has the lower index (P4)
    index = R.points_to_index_map(p1, R.FUSION_K, 640, 480)
    win = index[pix]
    tied = (win != i) & (p1[win, 2] == c[:, 2])
    assert tied.sum() == 867 and (win[tied] < i[tied]).all()
    # counted as collisions instead -- consecutive points (by index) of one pixel with bit-equal z, whether or not either wins it -- there are 869
    order = np.lexsort((i, pix))
    assert ((pix[order][1:] == pix[order][:-1]) & (c[order, 2][1:] == c[order, 2][:-1])).sum() == 869
    P, N, _ = R.depth_to_points(depth, 640, 480, R.FUSION_K, conv, want_normals=True)
    assert P.shape[0] == N.shape[0] == 113870
    assert R.depth_to_points(depth, 640, 480, R.FUSION_K, conv)[0].shape[0] == 118703


def test_frames_full_under_the_default_camera_is_all_ties(p1):
    """with K = 528 / 320 / 240 most projections of p1 are exact .5 ties: llround and rint part ways"""
    K = R.DEFAULT_K
    inv_z = F(1) / p1[:, 2]
    u = inv_z * R.dot3(K[0, 0], K[0, 1], K[0, 2], p1[:, 0], p1[:, 1], p1[:, 2])
    v = inv_z * R.dot3(K[1, 0], K[1, 1], K[1, 2], p1[:, 0], p1[:, 1], p1[:, 2])
    ties = (np.abs(u - np.trunc(u)) == 0.5) | (np.abs(v - np.trunc(v)) == 0.5)
    assert ties.sum() == 99563
    assert ((R.llround(u) != np.rint(u)) | (R.llround(v) != np.rint(v))).sum() == 60771
    # and the restatement follows llround: on a sample, the serial loop with Python's own rounding agrees
    sel = np.flatnonzero(ties)[:400]
    assert np.array_equal(R.points_to_index_map(p1[sel], K, 640, 480), R.points_to_index_map_literal(p1[sel], K, 640, 480))


def test_round_trip_on_a_ray_cast_scene():
    depth, K = R.raycast_scene()
    conv = R.Conv(R.U16, 1000.0)
    assert len(np.unique(depth)) > 100 and depth.min() > 0
    P, _, _ = R.depth_to_points(depth, 67, 45, K, conv)
    back, _ = R.points_to_depth_image(P, K, conv, 67, 45)
    assert np.array_equal(back.reshape(45, 67), depth)


def test_host_side_matrices():
    assert np.allclose(R.kinv(R.FUSION_K).astype(np.float64) @ R.FUSION_K.astype(np.float64), np.eye(3), atol=1e-6)
    L, t = R.to_cam(E_SMALL)
    back = R.transform(L, t, R.transform(E_SMALL[:3, :3], E_SMALL[:3, 3], np.array([[0.3, -0.2, 1.1]], F)))
    assert np.allclose(back, [[0.3, -0.2, 1.1]], atol=1e-5)


# ---- projective association -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_e", [0, 1])
def test_search_restatement_is_the_per_point_loop(with_e):
    rng = np.random.default_rng(6)
    dst = np.stack([rng.uniform(-0.5, 0.5, 400), rng.uniform(-0.4, 0.4, 400), rng.choice([0.75, 1.0, 1.25, -1.0], 400)], axis=1).astype(F)
    src = (dst[rng.integers(0, 400, 250)] + rng.normal(0, 0.005, (250, 3))).astype(F)
    src[::19] = np.nan
    K = np.array([[9.0, 0, 6.0], [0, 9.0, 4.5], [0, 0, 1]], F)
    E = E_SMALL if with_e else None
    T = R.small_E(angles=(0.01, 0.02, -0.01), t=(0.01, 0.0, -0.01))
    for r2 in (0.001, 0.05):
        got, lit = R.projective_search(dst, src, T, r2, K, 13, 10, E), R.projective_search_literal(dst, src, T, r2, K, 13, 10, E)
        assert np.array_equal(got[0], lit[0]) and np.array_equal(got[1].view(np.uint32), lit[1].view(np.uint32))
        assert 10 < (got[0] != R.EMPTY).sum() < 250


def test_search_counts_on_frames_full(p1):
    """p2 against p1 under the identity and the fusion camera"""
    p2 = np.load(GOLDEN)["p2"]
    counts = [int((R.projective_search(p1, p2, np.eye(4, dtype=F), F(r) ** 2, K=R.FUSION_K)[0] != R.EMPTY).sum()) for r in (0.01, 0.02, 0.1)]
    assert counts == [61494, 75079, 108515]


def test_host_rules_by_independent_arithmetic():
    """D2, P1 and the saturation of P5 are shared by the literal and the vectorised form: here they are checked exactly, against rational
    arithmetic rounded once"""
    from fractions import Fraction as Q

    def f32(q):      # a rational rounded once to f32 (through f64: 53 bits >= 2 * 24 + 2, no double rounding for these quotients and sums)
        return F(float(q))

    K = R.FUSION_K
    fx, fy, cx, cy = (Q(float(K[0, 0])), Q(float(K[1, 1])), Q(float(K[0, 2])), Q(float(K[1, 2])))
    want = np.array([[f32(1 / fx), 0, f32(-cx / fx)], [0, f32(1 / fy), f32(-cy / fy)], [0, 0, 1]], F)
    assert np.array_equal(R.kinv(K), want)
    L, t = R.to_cam(E_SMALL)
    e = [[Q(float(v)) for v in row] for row in E_SMALL]
    assert np.array_equal(L, E_SMALL[:3, :3].T)
    assert np.array_equal(t, np.array([f32(-(e[0][r] * e[0][3] + e[1][r] * e[1][3] + e[2][r] * e[2][3])) for r in range(3)], F))
    for c, b in ((-1.0, 0), (0.0, 0), (0.999, 254), (1.0, 255), (1.004, 255), (2.0, 255), (1e30, 255), (0.5, 127), (1 / 255, 1)):
        assert int(R.byte(np.array([c], F))[0]) == b, c


# ---- the crafted scenes of tests/test_gpu_projective_edges.py ----------------------------------------------------------------------
def tie_groups(pts, K=R.TIE_K, w=8, h=6):
    """per pixel the indices of its minimal-depth group (ascending)"""
    i, pix, c = R.project(pts, K, w, h)
    out = []
    for p in range(w * h):
        mem = i[pix == p]
        out.append(np.sort(mem[c[pix == p, 2] == c[pix == p, 2].min()]) if mem.size else mem)
    return out


def tie_group_span(pts, groups):
    """the smallest extent, over the groups and the two image axes, of a group's points"""
    return min(float(min(np.ptp(pts[g, 0]), np.ptp(pts[g, 1]))) for g in groups)


def test_tie_scene_ties_are_decided_by_index_alone():
    """rule P4 / S1 on a scene where the index order has nothing to do with any spatial order: 48 pixels, 64 points of bit-equal depth in
    each, one farther point behind them"""
    pts, grp = R.tie_scene()
    assert pts.shape == (48 * 65, 3)
    index = R.points_to_index_map(pts, R.TIE_K, 8, 6)
    assert np.array_equal(index, R.points_to_index_map_literal(pts, R.TIE_K, 8, 6)) and (index != R.EMPTY).all()
    u, v = R.computed_uv(pts, R.TIE_K)
    assert np.array_equal(u * 64, np.rint(u * 64)) and np.array_equal(v * 64, np.rint(v * 64))      # exact multiples of 1/64
    groups = tie_groups(pts)
    disagree = np.zeros(3, int)
    for p, g in enumerate(groups):
        assert g.size >= 64 and np.array_equal(g, np.flatnonzero(grp == p))      # (the far point is in no group)
        assert index[p] == g.min()
        q = pts[g]
        by_xyz, by_zyx = g[np.lexsort((q[:, 2], q[:, 1], q[:, 0]))][0], g[np.lexsort((q[:, 0], q[:, 1], q[:, 2]))][0]
        disagree += [by_xyz != index[p], by_zyx != index[p], g.max() != index[p]]
    print("tie scene: pixels where the first by (x, y, z), the first by (z, y, x), the highest index is not the winner:", disagree.tolist())
    assert (disagree >= 40).all()
    assert tie_group_span(pts, groups) == 62 / 64 / 4      # 62/64 of a pixel's footprint at z = 1
    # the other camera of the edge tests sees the same groups in its own frame
    pts0, grp0 = R.tie_scene(K=R.EDGE_K)
    index0 = R.points_to_index_map(pts0, R.EDGE_K, 8, 6)
    assert np.array_equal(index0, R.points_to_index_map_literal(pts0, R.EDGE_K, 8, 6)) and np.array_equal(grp0, grp)
    assert all(index0[p] == np.flatnonzero(grp0 == p).min() for p in range(48))


def test_boundary_points_land_where_rule_p3_says():
    w, h = 8, 6
    pts, want = R.boundary_points(w, h)
    # the computed projections ARE the values of the list (the generating formula alone rounds some of them away), on each of the three depths
    u, v = R.computed_uv(pts, R.EDGE_K)
    nu, nv = len(R.boundary_values(w)), len(R.boundary_values(h))
    for k in range(3):
        blk = k * (nu + nv)
        assert np.array_equal(u[blk:blk + nu], np.array(R.boundary_values(w), F)) and (v[blk:blk + nu] == 2).all()
        assert np.array_equal(v[blk + nu:blk + nu + nv], np.array(R.boundary_values(h), F)) and (u[blk + nu:blk + nu + nv] == 3).all()
    assert float(R.boundary_values(w)[1]) == -0.5 + 2.0 ** -25 and float(R.boundary_values(w)[7]) == 7.5 - 2.0 ** -21
    # rule P3, literally: -0.5 out, just above it pixel 0, -0.25 -> 0, 0.5 -> 1, 1.5 -> 2, 2.5 -> 3, w - 1, just below w - 0.5 -> w - 1, w - 0.5 out
    assert want[:nu].tolist() == [-1, 16, 16, 17, 18, 19, 23, 23, -1]
    assert want[nu:nu + nv].tolist() == [-1, 3, 3, 11, 19, 27, 43, 43, -1]
    assert (want[3 * (nu + nv):] == -1).all() and want.size - 3 * (nu + nv) == 6 + 20
    i, pix, _ = R.project(pts, R.EDGE_K, w, h)
    got = np.full(pts.shape[0], -1, np.int64)
    got[i] = pix
    assert np.array_equal(got, want)
    with np.errstate(all="ignore"):
        for k in range(pts.shape[0]):      # the serial loop, one point at a time
            ind = R._pixel_literal(pts[k], R.EDGE_K, w, h)
            assert (-1 if ind is None else ind) == want[k], (k, pts[k])
    assert np.array_equal(R.points_to_index_map(pts, R.EDGE_K, w, h), R.points_to_index_map_literal(pts, R.EDGE_K, w, h))
    # under the tie scene's own camera the float just above -0.5 is no point's projection: 4 x + 3.5 is a multiple of 2^-22 there
    just_above = np.nextafter(F(-0.5), F(0))
    for z in (1.0, 2.0, 0.5):
        assert R._coordinate_for(just_above, 0, F(0), z, R.TIE_K) is None and R._coordinate_for(just_above, 0, F(0), z, R.EDGE_K) is not None
        assert R._coordinate_for(F(-0.5), 0, F(0), z, R.TIE_K) is not None      # (the search itself works under that camera)
        x = R._coordinate_for(F(-0.5) + F(2.0 ** -22), 0, F(0), z, R.TIE_K)      # the nearest projection above -0.5 that exists there
        assert x is not None and R.computed_uv(np.array([[x, 0, z]], F), R.TIE_K)[0][0] == F(-0.5) + F(2.0 ** -22)
    # the searches agree on them too, as a source and inside a target
    dst = R.tie_scene(K=R.EDGE_K)[0]
    for a, b in ((dst, pts), (np.concatenate([pts, dst]), dst[:200])):
        got, lit = R.projective_search(a, b, np.eye(4, dtype=F), 3e38, R.EDGE_K, w, h), R.projective_search_literal(a, b, np.eye(4, dtype=F), 3e38, R.EDGE_K, w, h)
        assert np.array_equal(got[0], lit[0]) and np.array_equal(got[1].view(np.uint32), lit[1].view(np.uint32))


def test_organized_scene_projective_is_the_nearest_neighbour(orc):
    """one target point per pixel and a source a small fixed step away from every third of them: the projective search and an exhaustive
    nearest-neighbour search under the same radius name the same matches with the same values -- what lets a projective and a grid context be
    compared byte for byte (tests/test_gpu_projective_edges.py)"""
    P, N, S, K, w, h = R.organized_scene()
    assert P.shape == N.shape == (65 * 43, 3) and S.shape[0] == 932
    i, pix, _ = R.project(P, K, w, h)
    assert i.size == P.shape[0] and np.unique(pix).size == P.shape[0]      # one point per pixel
    si, spix, _ = R.project(S, K, w, h)
    assert si.size == S.shape[0] and np.array_equal(spix, pix[::3])      # (a) every source point on its own target point's pixel
    r2 = float(F(0.05) ** 2)
    I = np.eye(4, dtype=F)
    nn, val = R.projective_search(P, S, I, r2, K, w, h)
    lit = R.projective_search_literal(P, S, I, r2, K, w, h)
    assert np.array_equal(nn, lit[0]) and np.array_equal(val.view(np.uint32), lit[1].view(np.uint32))
    bi, bd = orc.nn_brute(P, S, r2)
    assert (nn != R.EMPTY).all() and np.array_equal(nn.astype(np.int64), bi) and np.array_equal(nn, np.arange(0, P.shape[0], 3))      # (b)
    assert np.array_equal(val.view(np.uint32), bd.view(np.uint32))


def test_the_oracle_update_accepts_an_empty_set(orc):
    P, N, S, _, _, _ = R.organized_scene()
    T0 = R.small_E(angles=(0.004, -0.003, 0.005), t=(0.004, -0.003, 0.002))
    none = np.zeros(0, np.int64)
    for metric in (0, 1):
        T, delta = orc.icp_update(P, N, S, T0, none, none, orc.make_params(metric=metric, max_iter=1, conv_tol=0.0, max_sq_dist=1e-14))
        assert np.array_equal(T, T0) and delta == 0.0
