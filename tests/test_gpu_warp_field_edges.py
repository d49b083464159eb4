"""GPU: the warp-field solver past one trip of every kernel and at the edges of its lists, through the C ABI,
against tests/_warp_refs.py and tests/_warp_affine_refs.py.  tests/test_gpu_warp_field*.py check the arithmetic on one graph shape
(204 to 400 nodes, k_ctrl = 4, k_reg = 8, ~2 000 arcs); here the graph changes and the arithmetic stays.

The trip boundaries (constants of csrc/warp_field.hip) and the tests that cross them:
  1 024 nodes    one block of WF_CG_THREADS: k_wf_cg_init / _update (node_dot), k_wf_gn_update, k_wf_max      (a) 1023 1024 1025, (b), (g)
  4 096 nodes    WF_NODE_BLOCKS x 4 waves: k_wf_gather_rhs, k_wf_apply_nodes                                   (a) 4095 4096 4097, (b), (g)
  65 536 nodes   WF_MAX_BLOCKS x WF_THREADS lanes: k_wf_to_transforms(_affine), k_wf_affine_start, k_wf_compose  (b), (g) at (b)'s lattice
  65 536 arcs    the same lanes: k_wf_arc_weights, k_wf_lin_arcs, the arc half of k_wf_apply_rows                (b)
  host code      n_arcs == 0, allocations of 0 elements, n_ctrl == 1                                            (a) 1, (c) k_reg = 1

Yardstick, unchanged from the two files above: the f64 restatement is "the exact answer", the f32 restatement "the reference as it
runs"; per component class -- a, b, c, tx, ty, tz for the rigid entry, each of the 12 stored values (the 3 x 3 row-major, then t) for
the affine entry, the maximum over the control nodes -- the device's error against the f64 restatement is at most 4 x the f32
restatement's, and the f32 restatement's is > 0 in every class.  Every estimate is one Gauss-Newton step of 1 or 2 CG iterations with
w_p2p = 0.1 (x1 = alpha M^-1 A^T b exercises A^T b, the diagonal and one application of the operator; x2 one more), with the other
parameters of the file the entry belongs to (w_reg = 200 rigid, 1 affine).

Graphs: _warp_refs.make_lattice_case (lists from a lattice, linear in the sizes).

Sizes 1 and 2 of (a).  A class of one or two nodes is one or two samples of a rounding error.  The device and the f32 restatement
form a source point's record (s_t or the rotation terms, the residuals) in f32 by the same expressions; the error that causes -- the
ROW FLOOR: the f32 restatement's own At and b, summed and solved in f64 (row_floor below) -- is common to both.  The restatement then
adds the roundings of its f32 sums, which in a class of one sample cancel the floor as often as they add to it: on the CPU, with 64
points, its error lies below a quarter of the floor in some class for 13 of 16 seeds at n = 1, and 4 x such an error asks the device for less
than exact sums of the same rows give.  So these two sizes take 4 096 source points, not 2 n_ctrl (over 4 096 terms the roundings of
the f32 sums outweigh the floor in the rigid classes, typically 5 to 100 times), and the first seed from n on for which, for both entries
and both iteration counts, the f32 restatement's error is at least HALF the row floor in every class (seeds 4 and 2).  Nothing but
the restatements enters that choice; the test asserts it.  The first MI355X runs, before this rule: with 64 points and seeds 1 and
2 the bound held in all classes but a at n = 1 and ty at n = 2 (rigid, 1 CG iteration: ratios 4.27 and 4.30; the f32 restatement at
0.31 and 0.32 of the floor); with 1 024 points in all but two at n = 1 (affine, 1 CG iteration: ratios 10.4 in L[1][2] and 4.2 in tx,
the f32 restatement at 0.10 and 0.24 of the floor), where the device's 12 errors equal to all nine printed digits those of a CPU
emulation of its stated arithmetic (f32 rows, f64 sums stored in f32, Eigen's f32 scalars): the device was right and the yardstick
a lucky draw.

CPU time of the largest restatement (66 049 nodes, 66 349 source points, 263 168 arcs; the explicit At At^T, one step of 2 CG
iterations, one core): rigid 0.3 s in f32 and 0.8 s in f64, affine 0.5 s and 1.2 s; Graph() itself 0.7 s.  No matrix-free operator
was needed.  The loop at that size has no restatement (its exact 1-NN is all-pairs): see test_loop_past_the_lane_trip.

What the tests catch, tried on a scratch build with one loop each cut short after its first trip (the two older files pass all four):
  k_wf_gather_rhs, the node loop         test_node_count_edges[4097-*], test_past_the_lane_per_item_trip, test_loop_past_the_node_trips
  k_wf_cg_update, the node_dot loop      test_node_count_edges[1025-*, 4095-*, 4096-*, 4097-*], the same two others (1024 passes)
  k_wf_lin_arcs                          test_past_the_lane_per_item_trip[rigid, affine]
  k_wf_to_transforms                     test_past_the_lane_per_item_trip[rigid], test_device_memory_and_repeatability[big-rigid]

Figures of the first MI355X run are recorded in the docstrings of the tests that measure them."""
import ctypes as C

import numpy as np
import pytest

import _warp_affine_refs as A
import _warp_refs as W
import test_gpu_warp_field as R
import test_gpu_warp_field_affine as RA
from cilantro_amd import capi
from test_gpu_warp_field import Field, cparams, last_error, transform_points
from test_gpu_warp_field_affine import AffineField

pytestmark = pytest.mark.gpu
F, D = np.float32, np.float64
HOST, DEVICE = capi.MEM_HOST, capi.MEM_DEVICE
NONE = W.NONE
KINDS = ("rigid", "affine")


def affine_errors(T, exact_tf):
    """the 12 classes: per stored value, the maximum over the nodes of |read-back - exact|, f64"""
    return np.abs(A.readback(T) - np.asarray(exact_tf, D).reshape(-1, 12)).max(0)


# per entry: the restatement, the file's parameters, the error classes, unknowns -> transforms, the resample restatement, transforms -> unknowns
ENTRY = {"rigid": dict(mod=W, prm=R.prm, errors=R.component_errors, to_T=W.to_transforms, resample=W.resample, readback=R.readback),
         "affine": dict(mod=A, prm=RA.prm, errors=affine_errors, to_T=A.to_transforms, resample=A.resample, readback=A.readback)}


def params(kind, max_cg, **kw):
    return ENTRY[kind]["prm"](max_gn_iter=1, max_cg_iter=max_cg, w_p2p=0.1, **kw)


# ---- cases and references, built once per module -----------------------------------------------------------------------------------
_CASES, _REFS = {}, {}


def cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def with_lists(c, **lists):
    """the case with some of its four list arrays replaced, and the graph of the new lists"""
    c = dict(c, **lists)
    c["graph"] = W.Graph(c["n_ctrl"], c["ctrl_idx"], c["ctrl_d2"], c["ctrl_kernel"], c["ctrl_sigma"], c["reg_idx"], c["reg_d2"], c["reg_kernel"], c["reg_sigma"])
    return c


def refs(c, key, kind, max_cg):
    """the f32 and f64 restatements of one estimate -> {dtype: (tforms_vec, stats)}; left unchanged by the tests that share them"""
    k = (key, kind, max_cg)
    if k not in _REFS:
        p = params(kind, max_cg)
        _REFS[k] = {t: ENTRY[kind]["mod"].estimate(c["graph"], t, c["dst"], c["dst_n"], c["src"], c["nn"], p) for t in (F, D)}
    return _REFS[k]


def device(c, kind, p):
    """create, estimate, resample the estimate, destroy -> (T, stats, dense)"""
    f = AffineField.of(c)
    try:
        T, st, _ = f.estimate(c["dst"], c["dst_n"], c["src"], c["nn"], p, rigid=kind == "rigid")
        dense = Field.resample(f, T) if kind == "rigid" else f.resample(T)
    finally:
        f.close()
    return T, st, dense


def check(c, key, kind, max_cg):
    """the yardstick, the two iteration counts and the resample of the result on one case -> (T, dense)"""
    e = ENTRY[kind]
    r = refs(c, key, kind, max_cg)
    T, st, dense = device(c, kind, params(kind, max_cg))
    e32, edev = e["errors"](e["to_T"](r[F][0], F), r[D][0]), e["errors"](T, r[D][0])
    with np.errstate(all="ignore"):
        print("\n%s %s cg=%d  f32 restatement error %s\n  device error %s\n  largest ratio %.3g" % (key, kind, max_cg, e32, edev, np.nanmax(edev / e32)))
    assert (e32 > 0).all(), e32
    assert (edev <= 4 * e32).all(), edev / e32
    assert (st.gn_iterations, st.cg_iterations_total) == (r[F][1]["gn_iterations"], r[F][1]["cg_iterations_total"]) == (1, max_cg)
    assert (T[:, 3] == [0, 0, 0, 1]).all() and (dense[:, 3] == [0, 0, 0, 1]).all()
    assert np.abs(dense - e["resample"](c["graph"], T, F)).max() < 2e-6
    return T, dense


# ---- a. node-count edges ---------------------------------------------------------------------------------------------------------
LATTICES = {1: (1, 1), 2: (2, 1), 63: (1, 63), 64: (8, 8), 65: (13, 5), 1023: (33, 31), 1024: (32, 32), 1025: (41, 25), 4095: (65, 63), 4096: (64, 64), 4097: (17, 241)}


def SOURCES(n):
    return 2 * n if n > 2 else 4096      # (the module docstring says why)


def row_floor(c, kind, max_cg):
    """(the f32 restatement's error, the error of its f32 rows alone) per class: At and b of the f32 restatement's first step, the
    normal equations formed and Eigen's CG run in f64"""
    e, p = ENTRY[kind], params(kind, max_cg)
    out = {}
    for t in (F, D):
        rec = []
        out[t] = e["mod"].estimate(c["graph"], t, c["dst"], c["dst_n"], c["src"], c["nn"], p, record=rec)[0], rec
    At, b = out[F][1][0][0].astype(D), out[F][1][0][1].astype(D)
    x = W.eigen_cg((At @ At.T).tocsc(), At @ b, p.cg_conv_tol, max_cg, D)[0]
    start = np.zeros(6 * c["n_ctrl"]) if kind == "rigid" else A.identity_start(c["n_ctrl"], D)
    return e["errors"](e["to_T"](out[F][0], F), out[D][0]), e["errors"](e["to_T"](start + x, D), out[D][0])


def yardstick_is_sound(c):
    return all((e32 >= 0.5 * floor).all() for e32, floor in (row_floor(c, kind, cg) for kind in KINDS for cg in (1, 2)))


def node_case(n):
    nx, ny = LATTICES[n]

    def build():
        for seed in range(n, n + 32):
            c = W.make_lattice_case(nx, ny, 2, 5, extra=SOURCES(n) - n, seed=seed)
            if n > 2 or yardstick_is_sound(c):
                return dict(c, seed=seed)

    return cached(("nodes", n), build)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", list(LATTICES))
def test_node_count_edges(n, kind, max_cg):
    """k_ctrl = 2, k_reg = 5, 2 n source points (4 096 at n = 1 and 2, and the seed the module docstring's rule picks).  n = 1: no arcs, a list of [0, NONE] per point, one node every
    point names.
    First MI355X run, largest ratio device / f32 restatement over the classes (1 CG iteration, 2):
      n        rigid 1, 2      affine 1, 2          n        rigid 1, 2      affine 1, 2          n        rigid 1, 2      affine 1, 2
      1        0.04  0.23      1.00  1.00           65       1.43  0.56      1.00  1.10           4095     0.83  0.53      1.01  1.01
      2        1.00  0.22      1.04  1.00           1023     1.45  1.56      1.00  1.04           4096     1.10  1.25      1.01  1.02
      63       1.00  1.11      1.01  1.02           1024     0.75  0.34      1.06  1.03           4097     0.74  0.41      1.20  1.08
      64       1.00  1.30      1.01  1.05           1025     0.70  0.52      1.00  1.06
    (the largest errors: f32 restatement 6e-9..7e-8, device 1e-11..1e-9 rigid; both 6e-8, half an ulp of the stored 1 + x, affine from 63 nodes on)"""
    c = node_case(n)
    assert c["n_ctrl"] == n and len(c["src"]) == SOURCES(n)
    if n == 1:
        assert len(c["graph"].arc_s) == 0 and (c["ctrl_idx"] == [0, NONE]).all()
    if n <= 2:
        assert c["seed"] == {1: 4, 2: 2}[n] and yardstick_is_sound(c)
    check(c, ("nodes", n), kind, max_cg)


# ---- b. past the lane-per-item trip ----------------------------------------------------------------------------------------------
def big_case():
    return cached("big", lambda: W.make_lattice_case(257, 257, 1, 5, extra=300, seed=7, ctrl_kernel=W.UNITY, reg_kernel=W.RBF))


@pytest.mark.parametrize("kind", KINDS)
def test_past_the_lane_per_item_trip(kind):
    """257 x 257 = 66 049 nodes (258 x 256 + 1), 263 168 arcs, k_ctrl = 1 (Unity), RBF arcs, 66 349 source points, 2 CG
    iterations; then the resample (in check) and the per-point transform of the source by it, bit for bit.
    First MI355X run:
      rigid: f32 restatement at most 7.9e-8 over the classes, device at most 1.6e-10, largest ratio 0.14;
      affine: f32 restatement at most 6.2e-8, device 6.0e-8, largest ratio 0.99"""
    c = big_case()
    assert c["n_ctrl"] > 65536 and len(c["graph"].arc_s) > 65536 and c["n_ctrl"] % 256 != 0 and len(c["src"]) == c["n_ctrl"] + 300
    T, dense = check(c, "big", kind, 2)
    assert transform_points(dense, c["src"]).tobytes() == W.transform_points(dense, c["src"]).tobytes()


# ---- c. list widths and padding --------------------------------------------------------------------------------------------------
WIDTHS = [(1, 1), (1, 2), (2, 32), (32, 2), (32, 32)]
KERNELS = [(W.UNITY, W.UNITY), (W.UNITY, W.RBF), (W.RBF, W.UNITY), (W.RBF, W.RBF)]


def width_case(k_ctrl, k_reg, ck=W.RBF, rk=W.RBF):
    return cached(("widths", k_ctrl, k_reg, ck, rk), lambda: W.make_lattice_case(20, 15, k_ctrl, k_reg, extra=300, seed=31, ctrl_kernel=ck, reg_kernel=rk))


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k_ctrl, k_reg", WIDTHS)
def test_list_widths(k_ctrl, k_reg, kind, max_cg):
    """300 nodes, 600 source points.  k_reg = 1: rows of [i] only, n_arcs == 0 on a graph with many nodes (the system is its data
    term alone; the device skips k_wf_lin_arcs and allocates arc buffers of 0 elements).  k = 32 is the widest list the ABI takes.
    First MI355X run, largest ratio (1 CG iteration, 2):
      (k_ctrl, k_reg)   rigid 1, 2      affine 1, 2
      (1, 1)            0.81  0.67      1.38  1.67      (no arcs: the affine system is loose, both errors reach 1.3e-5 and 2.2e-5)
      (1, 2)            0.81  1.09      1.01  1.02
      (2, 32)           0.75  0.62      1.01  1.28
      (32, 2)           0.54  0.14      2.85  1.98      (k_ctrl = 32, affine: the device blends the 12 values in list order, the restatement in
      (32, 32)          0.26  0.16      3.01  1.76       the reference's order, by node index: two roundings of a 32-term f32 sum; off the diagonal 1.5 to 3 times the error)"""
    c = width_case(k_ctrl, k_reg)
    assert c["n_ctrl"] == 300 and c["ctrl_idx"].shape == (600, k_ctrl) and c["reg_idx"].shape == (300, k_reg)
    assert (len(c["graph"].arc_s) == 0) == (k_reg == 1)
    check(c, ("widths", k_ctrl, k_reg), kind, max_cg)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ck, rk", KERNELS)
def test_both_kernels_on_both_list_families(ck, rk, kind):
    """(k_ctrl, k_reg) = (4, 8), 2 CG iterations.  First MI355X run, largest ratio:
      Unity/Unity 0.75 rigid, 1.00 affine; Unity/RBF 0.95, 1.00; RBF/Unity 0.89, 1.62; RBF/RBF 0.39, 1.60"""
    check(width_case(4, 8, ck, rk), ("kernels", ck, rk), kind, 2)


def holes_case():
    """NONE in the middle of lists: slot 1 of every third control list, slot 2 of every fourth regularisation row, and slots 1 and 2
    of every 17th control list (the survivor is the last slot)"""
    def build():
        c = width_case(4, 8)
        ci, ri = c["ctrl_idx"].copy(), c["reg_idx"].copy()
        ci[::3, 1] = NONE
        ci[::17, 1:3] = NONE
        ri[::4, 2] = NONE
        return with_lists(c, ctrl_idx=ci, reg_idx=ri)

    return cached("holes", build)


def ownerless_case():
    """every fifth regularisation row has NONE where its owner stands: the row contributes no arc (the other rows still name its node)"""
    def build():
        c = width_case(4, 8)
        ri = c["reg_idx"].copy()
        ri[::5, 0] = NONE
        return with_lists(c, reg_idx=ri)

    return cached("ownerless", build)


def orphan_case():
    """every 55th source point from 7 on (none of the unmatched ones: those stand at 5 + 11 i) has a control list of NONE only and a correspondence: the reference gives such a point an
    empty list and a total of 0 (warp_field_estimation.hpp:1456-1465), so both weights are 0 (:1593-1596, :1687-1690), its rows of At
    are empty and its entries of b are 0: it counts as a correspondence and contributes nothing; the resample leaves it the identity"""
    def build():
        c = width_case(4, 8)
        ci = c["ctrl_idx"].copy()
        ci[7::55] = NONE
        return with_lists(c, ctrl_idx=ci)

    return cached("orphans", build)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_none_in_the_middle_of_lists(kind, max_cg):
    """First MI355X run, largest ratio (1 CG iteration, 2):
      rigid 1.49, 0.69; affine 1.05, 1.19"""
    c, base = holes_case(), width_case(4, 8)
    assert (c["ctrl_idx"][::3, 1] == NONE).all() and (c["ctrl_idx"][::3, 2] != NONE).any() and len(c["graph"].arc_s) < len(base["graph"].arc_s)
    check(c, "holes", kind, max_cg)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_without_an_owner_give_no_arc(kind, max_cg):
    """First MI355X run, largest ratio (1 CG iteration, 2):
      rigid 1.30, 0.78; affine 1.49, 1.31"""
    c, base = ownerless_case(), width_case(4, 8)
    gone = int((base["reg_idx"][::5, 1:] != NONE).sum())
    assert gone > 0 and len(c["graph"].arc_s) == len(base["graph"].arc_s) - gone
    check(c, "ownerless", kind, max_cg)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_points_with_an_empty_control_list_contribute_nothing(kind, max_cg):
    """the estimate equals, bit for bit, the one in which those points have no correspondence either, and meets the yardstick.
    First MI355X run, largest ratio (1 CG iteration, 2):
      rigid 1.34, 1.05; affine 1.02, 1.57"""
    c = orphan_case()
    orphans = np.arange(7, len(c["src"]), 55)
    assert (c["nn"][orphans] != NONE).all() and (c["graph"].total[orphans] == 0).all()
    T, dense = check(c, "orphans", kind, max_cg)
    assert (dense[orphans] == np.eye(4, dtype=F)).all()
    nn = c["nn"].copy()
    nn[orphans] = NONE
    T2, st2, _ = device(dict(c, nn=nn), kind, params(kind, max_cg))
    assert T2.tobytes() == T.tobytes()


# ---- d. unbalanced gather --------------------------------------------------------------------------------------------------------
def hub_case():
    """129 nodes (43 x 3), 5 000 source points, Unity control weights: every point lists node 0, then its nearest lattice node other
    than 0 and other than the nodes with index % 5 == 2, which no point names"""
    def build():
        c = W.make_lattice_case(43, 3, 3, 5, extra=5000 - 129, seed=43, ctrl_kernel=W.UNITY)
        near = c["ctrl_idx"].astype(np.int64)
        ok = (near != 0) & (near % 5 != 2)
        assert ok.any(1).all()
        second = near[np.arange(len(near)), ok.argmax(1)]
        ci = np.stack([np.zeros(len(near), np.int64), second], 1).astype(np.uint32)
        cd = np.stack([W.d2_pairs(c["src"], c["ctrl"][ci[:, 0]]), W.d2_pairs(c["src"], c["ctrl"][ci[:, 1]])], 1)
        return with_lists(c, ctrl_idx=ci, ctrl_d2=cd)

    return cached("hub", build)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_unbalanced_gather(kind, max_cg):
    """node 0's inverse list has 5 000 entries (79 trips of its wave), the others at most 71, 26 nodes none.
    First MI355X run, largest ratio (1 CG iteration, 2):
      rigid 0.05, 0.16 (f32 restatement 5e-8, device 1e-10); affine 1.00, 1.00"""
    c = hub_case()
    named = np.bincount(c["ctrl_idx"].reshape(-1), minlength=129)
    assert len(c["src"]) == 5000 and named[0] == 5000 and (named[np.arange(129) % 5 == 2] == 0).all() and (named == 0).sum() == 26 and named[1:].max() < 1000
    check(c, "hub", kind, max_cg)


# ---- e. off-origin ---------------------------------------------------------------------------------------------------------------
OFFSET = np.array([100.0, -50.0, 30.0])


def origin_case():
    def build():
        c = W.make_case()
        c["nn"] = W.nearest(c["dst"], c["src"], c["max_sq"])
        return c

    return cached("origin", build)


def offset_case():
    """make_case() moved by (100, -50, 30) m: source, target and nodes in f32; the same lists and correspondences, the squared
    distances of the listed pairs from the moved f32 coordinates through the pinned expression"""
    def build():
        c = origin_case()
        src, dst, ctrl = ((c[k].astype(D) + OFFSET).astype(F) for k in ("src", "dst", "ctrl"))
        ci, ri = np.where(c["ctrl_idx"] == NONE, 0, c["ctrl_idx"]).astype(np.int64), np.where(c["reg_idx"] == NONE, 0, c["reg_idx"]).astype(np.int64)
        cd = np.where(c["ctrl_idx"] == NONE, F(0), W.d2_pairs(src[:, None, :], ctrl[ci]))
        rd = np.where(c["reg_idx"] == NONE, F(0), W.d2_pairs(ctrl[:, None, :], ctrl[ri]))
        return with_lists(dict(c, src=src, dst=dst, ctrl=ctrl), ctrl_d2=cd.astype(F), reg_d2=rd.astype(F))

    return cached("offset", build)


@pytest.mark.parametrize("max_cg", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
def test_off_origin(kind, max_cg):
    """the yardstick against the f64 restatement of the moved inputs (f32 cancellation hits the f32 restatement as well), and the
    device's error against 4 x the f32 restatement's error AT THE ORIGIN times the ratio of the two f32 restatement errors, per class:
    the device loses no more precision to the offset than the reference does.
    First MI355X run (f32 restatement error moved / at the origin, device error moved / at the origin, largest over the classes):
      rigid, 1 CG iteration: f32 restatement 0.013 to 0.95 times its error at the origin over the classes, device 0.014 to 0.18 times; 2: 0.019
      to 4.1 and 0.011 to 0.19 (the step is smaller off the origin: a rotation about the origin moves a point 100 m away by 100 m per radian);
      affine, 1: f32 restatement 1.0 to 132 times, device 1.0 to 106 times; 2: 1.05 to 181 and 1.08 to 140.  Largest ratio device / f32
      restatement on the moved pair: rigid 0.66, 0.37; affine 1.69, 1.13"""
    e = ENTRY[kind]
    c0, c1 = origin_case(), offset_case()
    assert c1["n_ctrl"] == 286 and np.abs(c1["src"].mean(0) - OFFSET).max() < 1.0
    r0, r1 = refs(c0, "origin", kind, max_cg), refs(c1, "offset", kind, max_cg)
    T1, _ = check(c1, "offset", kind, max_cg)
    T0, _, _ = device(c0, kind, params(kind, max_cg))
    e32_0, e32_1 = e["errors"](e["to_T"](r0[F][0], F), r0[D][0]), e["errors"](e["to_T"](r1[F][0], F), r1[D][0])
    edev_0, edev_1 = e["errors"](T0, r0[D][0]), e["errors"](T1, r1[D][0])
    print("\noff-origin %s cg=%d  f32 growth %s\n  device growth %s" % (kind, max_cg, e32_1 / e32_0, edev_1 / edev_0))
    assert (e32_0 > 0).all() and (edev_0 <= 4 * e32_0).all()
    assert (edev_1 <= 4 * e32_0 * (e32_1 / e32_0)).all()


# ---- f. device memory and repeatability ------------------------------------------------------------------------------------------
def live():
    out = (C.c_ulonglong * 2)()
    assert capi.load().cilhip_debug_live_allocations(out) == capi.OK
    return out[0], out[1]


def run_in(mem, c, kind, p):
    """create, estimate, resample, destroy with every array in `mem` -> (ctrl transforms, stats, dense transforms) as the ABI wrote them"""
    import torch

    L, h = capi.load(), C.c_void_p()
    est, res = (L.cilhip_warp_field_estimate3f, L.cilhip_warp_field_resample3f) if kind == "rigid" else (L.cilhip_warp_field_estimate_affine3f, L.cilhip_warp_field_resample_affine3f)
    host = [np.ascontiguousarray(c[k], t) for k, t in (("ctrl_idx", np.uint32), ("ctrl_d2", F), ("reg_idx", np.uint32), ("reg_d2", F), ("dst", F), ("dst_n", F), ("src", F), ("nn", np.uint32))]
    n_src, n_ctrl = len(c["src"]), c["n_ctrl"]
    ctrl_out, dense_out = np.full(16 * n_ctrl, 7, F), np.full(16 * n_src, 7, F)
    if mem == DEVICE:
        dev = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in host]
        d_ctrl, d_dense = torch.from_numpy(ctrl_out.copy()).cuda(), torch.from_numpy(dense_out.copy()).cuda()
        torch.cuda.synchronize()
        ptr, p_ctrl, p_dense = [t.data_ptr() for t in dev], d_ctrl.data_ptr(), d_dense.data_ptr()
    else:
        ptr, p_ctrl, p_dense = [a.ctypes.data for a in host], ctrl_out.ctypes.data, dense_out.ctypes.data
    st = capi.WarpStats()
    rc = L.cilhip_warp_field_create(0, n_src, n_ctrl, ptr[0], ptr[1], c["ctrl_idx"].shape[1], c["ctrl_kernel"], float(c["ctrl_sigma"]), ptr[2], ptr[3], c["reg_idx"].shape[1],
                                    c["reg_kernel"], float(c["reg_sigma"]), mem, C.byref(h))
    assert rc == capi.OK, last_error(L)
    try:
        assert est(h, ptr[4], ptr[5], len(c["dst"]), ptr[6], ptr[7], mem, C.byref(cparams(p)), p_ctrl, C.byref(st)) == capi.OK, last_error(L)
        assert res(h, p_ctrl, p_dense, mem) == capi.OK, last_error(L)
    finally:
        L.cilhip_warp_field_destroy(h)
    if mem == DEVICE:
        torch.cuda.synchronize()
        ctrl_out, dense_out = d_ctrl.cpu().numpy(), d_dense.cpu().numpy()
    return ctrl_out.tobytes(), bytes(st), dense_out.tobytes()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["nodes_1025", "big"])
def test_device_memory_and_repeatability(which, kind):
    """create, estimate and resample with MEM_DEVICE on torch tensors write the bytes MEM_HOST writes; a second run writes them again
    (sums of fixed order, no floating-point atomics); the library's live allocations return to where they started"""
    c = big_case() if which == "big" else node_case(1025)
    p = params(kind, 2)
    before = live()
    a = run_in(HOST, c, kind, p)
    assert live() == before
    b = run_in(DEVICE, c, kind, p)
    assert live() == before
    a2 = run_in(HOST, c, kind, p)
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert a == a2
    T = np.frombuffer(a[0], F).reshape(-1, 4, 4)
    assert not (T == np.eye(4, dtype=F)).all() and not (T == 7).any() and not (np.frombuffer(a[2], F) == 7).any()


# ---- g. the loop past the node trips ---------------------------------------------------------------------------------------------
def dense_style(c):
    """every source point its own control node: the source is the nodes' jittered copies, ctrl_idx[i] = i, k_ctrl = 1, Unity"""
    n = c["n_ctrl"]
    assert len(c["src"]) == n
    return with_lists(dict(c, ctrl_kernel=W.UNITY), ctrl_idx=np.arange(n, dtype=np.uint32)[:, None], ctrl_d2=np.zeros((n, 1), F))


def loop_case():
    return cached("loop", lambda: dense_style(W.make_lattice_case(60, 70, 1, 6, seed=60, ctrl_kernel=W.UNITY)))


def loop_prm(kind):
    return ENTRY[kind]["prm"](max_gn_iter=1, max_cg_iter=2, w_p2p=0.1)


_LOOPS = {}


def loop_refs(kind):
    if kind not in _LOOPS:
        c = loop_case()
        _LOOPS[kind] = {t: ENTRY[kind]["mod"].icp_loop(c["graph"], t, c["dst"], c["dst_n"], c["src"], loop_prm(kind), 2, 0.0, c["max_sq"]) for t in (F, D)}
    return _LOOPS[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_loop_past_the_node_trips(kind):
    """cilhip_warp_field_icp_run(_affine), n_ctrl = n_src = 4 200 (60 x 70) dense style, k_reg = 6, two outer iterations of one
    Gauss-Newton step of 2 CG iterations (conv_tol = 0: both run): the composed control transforms against the loop restatement by
    the yardstick; the iteration count; the returned last_delta_norm (the root of max_delta_sq, k_wf_compose and k_wf_max past 1 024
    and 4 096 nodes) within 4 x the f32 restatement's own error against the f64 one, that error taken as at least one rounding of
    the returned f32 value.
    First MI355X run:
      rigid: f32 restatement 5.4e-8 5.6e-8 4.5e-8 5.1e-9 1.9e-9 5.8e-9, device 4.3e-10 6.7e-10 2.9e-10 6.3e-10 2.4e-10 8.4e-10 (largest
      ratio 0.15); last_delta_norm 1.016872345e-3 (f64), 1.016873517e-3 (f32), 1.016872586e-3 (device).  affine: largest ratio 1.69 (L[0][1], 1.9e-9
      against 1.1e-9; the three diagonal classes 1.00, 1.12, 1.12 at 1.6e-7 to 2.0e-7); last_delta_norm 1.753317058e-3, 1.753309043e-3, 1.753309043e-3.
      4 200 correspondences in both iterations of all."""
    e = ENTRY[kind]
    c, r = loop_case(), loop_refs(kind)
    assert c["n_ctrl"] == 4200 and c["reg_idx"].shape[1] == 6
    assert r[F]["ncorr"] == r[D]["ncorr"] == [4200, 4200]
    f = AffineField.of(c)
    try:
        got = RA.icp_run(c, f, loop_prm(kind), 2, conv_tol=0.0, rigid=kind == "rigid")
    finally:
        f.close()
    exact = e["readback"](r[D]["T"])
    e32, edev = e["errors"](r[F]["T"].astype(F), exact), e["errors"](got["T"], exact)
    d32, d64 = r[F]["last_delta_norm"], r[D]["last_delta_norm"]
    print("\nloop %s  f32 restatement error %s\n  device error %s\n  largest ratio %.3g\n  last_delta_norm f64 %.9e f32 %.9e device %.9e" % (kind, e32, edev, (edev / e32).max(), d64, d32, got["last_delta_norm"]))
    assert (e32 > 0).all() and (edev <= 4 * e32).all(), edev / e32
    assert got["iterations"] == r[F]["iterations"] == 2 and got["ncorr"] == r[F]["ncorr"][-1]
    assert abs(got["last_delta_norm"] - d64) <= 4 * max(abs(d32 - d64), float(np.spacing(F(d64))) / 2)
    assert np.abs(got["dense"] - e["resample"](c["graph"], got["T"], F)).max() < 2e-6


def compose_pinned(T_iter, T):
    """k_wf_compose on the host, f32, every operation rounded once: T_iter * T with the last row (0, 0, 0, 1), and per node
    |R_iter - I|_F^2 + |t_iter|^2 summed column by column, then t"""
    a, b = np.asarray(T_iter, F), np.asarray(T, F)
    out = np.zeros_like(b)
    for col in range(4):
        for r in range(3):
            out[:, r, col] = ((a[:, r, 0] * b[:, 0, col] + a[:, r, 1] * b[:, 1, col]) + a[:, r, 2] * b[:, 2, col]) + (a[:, r, 3] if col == 3 else F(0))
    out[:, 3, 3] = 1
    d2 = np.zeros(len(a), F)
    for col in range(3):
        for r in range(3):
            v = a[:, r, col] - F(1 if r == col else 0)
            d2 = d2 + v * v
    for r in range(3):
        d2 = d2 + a[:, r, 3] * a[:, r, 3]
    return out, d2


@pytest.mark.parametrize("kind", KINDS)
def test_loop_past_the_lane_trip(kind):
    """the loop at the 66 049-node lattice of (b), dense style: k_wf_compose past 65 536 nodes.  The loop restatement needs an exact
    1-NN of 66 049 points in 66 049 on the CPU (all pairs) and is not run at this size; this test uses the invariants that need none:
    the two-iteration result equals, bit for bit, the composition -- in f32 on the host with the kernel's pinned expression -- of the
    two single-iteration results obtained by hand (the context's search, the estimate entry, the resample entry and the per-point
    transform, which the tests above measure), last_delta_norm is the root of the hand-made maximum, and a second run gives the bytes
    of the first.
    First MI355X run: 66 049 correspondences in both iterations; the delta by hand 5.2466e-3 then 1.9416e-3 (rigid), 4.3364e-3 then
    1.4136e-3 (affine); every comparison bit for bit."""
    from cilantro_amd.icp import Context

    c = cached("big_dense", lambda: dense_style(W.make_lattice_case(257, 257, 1, 5, seed=8, ctrl_kernel=W.UNITY)))
    assert c["n_ctrl"] > 65536 and c["n_ctrl"] % 256 != 0
    p, rigid, eye = loop_prm(kind), kind == "rigid", np.eye(4, dtype=F)
    f, ctx = AffineField.of(c), Context(0)
    try:
        ctx.set_target(c["dst"], c["dst_n"])
        ctx.set_source(c["src"])
        got = RA.icp_run(c, f, p, 2, conv_tol=0.0, ctx=ctx, rigid=rigid)
        again = RA.icp_run(c, f, p, 2, conv_tol=0.0, ctx=ctx, rigid=rigid)
        resample = (lambda T_: Field.resample(f, T_)) if rigid else f.resample
        T, steps = np.tile(eye, (c["n_ctrl"], 1, 1)), []
        dense = resample(T)
        for _ in range(2):
            warped = transform_points(dense, c["src"])
            ctx.set_source(warped)
            ncorr = ctx.find_correspondences(eye, float(c["max_sq"]))
            nn = ctx.get_nn()[0].copy()
            T_iter, st, _ = f.estimate(c["dst"], c["dst_n"], warped, nn, p, rigid=rigid)
            T, d2 = compose_pinned(T_iter, T)
            dense = resample(T)
            steps.append((ncorr, float(np.sqrt(d2.max()))))
    finally:
        ctx.close(); f.close()
    print("\nloop at %d nodes, %s: by hand (ncorr, delta) %s; the loop %d iterations, ncorr %d, delta %.9e" % (c["n_ctrl"], kind, steps, got["iterations"], got["ncorr"], got["last_delta_norm"]))
    assert steps[0][0] > 65536 and steps[0][1] > 0 and steps[1][1] > 0
    assert got["iterations"] == 2 and got["ncorr"] == steps[1][0]
    assert got["T"].tobytes() == T.tobytes() and got["dense"].tobytes() == dense.tobytes()
    assert F(got["last_delta_norm"]) == np.sqrt(d2.max())
    assert got["bytes"] == again["bytes"] and (got["last_delta_norm"], got["ncorr"]) == (again["last_delta_norm"], again["ncorr"])
