"""GPU: the kernels of mean shift (3-D and N-d), N-d connected components and the convex hull that are launched with a CAPPED grid and walk the
rest of their input in a grid-stride loop, each driven past its cap.  The second trip of such a loop is where a wrong stride, a 32-bit index,
a wave-wide append inside a non-uniform loop or a cursor that is not carried over goes wrong, and no smaller run can see it.  Every expected
result is a closed form of tests/_trip_refs.py (O(n) numpy in f64 on exactly representable inputs, pinned against the suite's yardsticks at
small sizes by tests/test_trip_refs_cpu.py); integers are compared with np.array_equal and floats bit for bit -- on these lattices every
f64 sum is exact in any order.  (k_pca_project / k_pca_reconstruct: the 600 001-row case of tests/test_gpu_pca.py.)

Which case drives which kernel past its cap, and what a skipped (or repeated, or mis-strided) second trip would change in the output:

cap 2048 blocks x 256 lanes = 524 288 items per trip (prim_blocks)
  k_ms_seed_keys     shift_and_group, *_non_finite_rows, *_own_seeds (540 000 seeds over a grid).  The keys and list entries of the seeds from
                     524 288 on: those seeds would not be in the first active list (or twice), and `shifted` would keep them where they came.
  k_ms_group_init    every 3-D case.  state / lead_of of the seeds from 524 288 on and their entries of U, appended per wave inside the loop: such
                     a seed would be nobody's member -- `labels`, `offsets`, `members` differ (every_seed_a_leader: 12 clusters short).
  k_iota (mean_shift.hip)   no_finite_point: the first active list without a grid.  The seeds from 524 288 on would not be shifted to NaN.
  k_points_clean     *_non_finite_rows: all six non-finite rows lie at 524 288 or above.  The clean copy of those rows and the finite count:
                     the grid would hold unwritten rows and the late seeds' means differ.
  k_ms_leader_flags  every grouped case, ns + 1 words.  every_seed_a_leader: the flags from 524 288 on are all ones and the closing word is the
                     last of the second trip -- the cluster count (the scan's last word) would be short; grouping_alone: the count again.
  k_ms_labels        every grouped case: `labels` from 524 288 on.
  group_by_label     every case.  k_iota: `members` holds every index once; k_run_offsets: the run starts found at sorted positions from
                     524 288 on (grouping_alone: the offsets of the clusters from about 15 900 on; every_seed_a_leader: offsets[524 288:]);
                     the sort's key_bits: 15 bits (16 400 labels) and 20 bits (524 300 labels) where the suite had 9.
  k_iota (mean_shift_nd.hip)   nd_shift: the first active list -- the seeds from 524 288 on would stay where they came.
  k_msn_group_init   nd_grouping_alone, nd_shift, nd_modes_past_the_wave_cap (ns + 1 words): state, lead_of and the flags the scan packs U from.
  k_msn_pack         the same cases: U's coordinates and indices from 524 288 on -- those seeds would never be claimed, `labels` differ.
  k_iota / k_ms_modes<5> (N-d, ungrouped)   nd_tolerance_zero: labels are the indices; 524 300 clusters.
  k_ccn_extent       ccn_chain: the count of finite rows m is summed over both trips -- 75 713 rows short, the rows last in sweep order would be
                     left out of the stream and stay singletons.  (The axis it picks is reported and asserted too.)
  k_ccn_sort_keys, k_iota (components_nd.hip: parents, sort values), k_ccn_gather   ccn_chain: keys, parents and sorted rows from 524 288 on; a
                     row without its key or its sorted copy joins the wrong segment or none: `labels` and the five sizes differ.
cap 4096 blocks x 4 waves = 16 384 waves per trip
  k_ms_claim         grouping_alone / shift_and_group: 16 400 leaders elected in ONE round (asserted: rounds == 1), the last 16 claimed in a second
                     trip -- skipped, they would stay undecided and the grouping would need more rounds or lose their members;
                     every_seed_a_leader: 524 300 leaders, 33 trips.
  k_ms_modes<3>      the same cases: the modes of the clusters from 16 384 on, compared bit for bit.
  k_ms_modes<2>      nd_modes_past_the_wave_cap (16 400 clusters of 32 or 33 members);  k_ms_modes<5>: nd_tolerance_zero.
cap 1024 blocks x 256 lanes = 262 144 points per trip
  k_hull_seed<3>, <2>   hull_late: all five non-finite rows (n_nonfinite), the largest |coordinate| (the band: a smaller one is asserted to change
                     tol, test_trip_refs_cpu.py) and thirteen of the fourteen (seven of the eight) extreme points lie in the second trip; the
                     extreme of the diagonal ties across the trips and must be reported as row 7.  With the late seeds the first polytope holds
                     the whole inner ball (it contains the octahedron / square of the axis points, inradius > 0.5), so the first round leaves
                     at most the late finite rows: survivors_first_round is asserted against that.

Not here, on purpose: k_list_offsets of knn_nd.hip runs only with more than one slice, and nd_slices() gives one slice as soon as there are
more than ND_TARGET_BLOCKS x 256 queries -- its second trip cannot be reached by any call.
"""
import functools

import numpy as np
import pytest

import _hull_refs as RH
import _trip_refs as T
from test_gpu_components_nd import run as ccn_run
from test_gpu_convex_hull import bits, capi_hull, check as hull_check
from test_gpu_mean_shift import run as ms_run
from test_gpu_mean_shift_nd import run as msn_run

pytestmark = pytest.mark.gpu

NS, K = 540_000, 16_400      # past 524 288 seeds and past 16 384 clusters, each with a margin of a few thousand / a few
NS_ND = T.PRIM_TRIP + 12      # 524 300
ARRAYS = ("shifted", "labels", "offsets", "members", "modes")


@pytest.fixture(scope="module")
def cl():
    from cilantro_amd import clustering

    return clustering


clustered = functools.lru_cache(maxsize=None)(T.clustered)      # each cloud is built once and shared; nothing writes to it
spread = functools.lru_cache(maxsize=None)(T.spread)


def same(got, want, iterations):
    for k in ARRAYS:
        a, b = got[k], want[k]
        assert a.shape == b.shape, (k, a.shape, b.shape)
        if k in ("shifted", "modes"):      # bit for bit; where a NaN is expected, any NaN
            nan = np.isnan(b)
            assert np.array_equal(np.isnan(a), nan), (k, int((np.isnan(a) != nan).sum()))
            assert np.array_equal(bits(a)[~nan], bits(b)[~nan]), (k, int((bits(a)[~nan] != bits(b)[~nan]).sum()))
        else:
            assert np.array_equal(a, b), (k, int((a != b).sum()))
    assert got["iterations"] == iterations


def every_seed_its_own_cluster(got, ns):
    assert np.array_equal(got["labels"], np.arange(ns)) and np.array_equal(got["offsets"], np.arange(ns + 1)) and np.array_equal(got["members"], np.arange(ns))


# ---- mean shift, 3-D ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_mem", [False, True])
def test_ms3_grouping_alone(cl, device_mem):
    c = clustered(NS, K)
    assert NS > T.PRIM_TRIP and K > T.WAVE_TRIP and int(c["offsets"][T.WAVE_TRIP]) > T.PRIM_TRIP      # run starts in the second trip of k_run_offsets
    want = T.clustered_forms(c, 0)
    got = ms_run(cl, np.zeros((3, 3), np.float32), c["points"], 1.0, 0, c["tol"], device_mem=device_mem)
    same(got, want, 0)
    assert np.array_equal(got["members"][got["offsets"][:-1]], c["leaders"]) and got["modes"].shape == (K, 3)
    assert got["stats"]["rounds"] == 1      # every leader is elected, and claims its members, in one round: 16 400 waves of k_ms_claim
    print("grouping", got["stats"])


def test_ms3_every_seed_a_leader(cl):
    seeds = spread(NS_ND, 3)
    got = ms_run(cl, np.zeros((3, 3), np.float32), seeds, 1.0, 0, 0.0)
    every_seed_its_own_cluster(got, NS_ND)
    assert got["iterations"] == 0 and bits(got["shifted"]).tobytes() == bits(seeds).tobytes() and bits(got["modes"]).tobytes() == bits(seeds).tobytes()
    assert got["stats"]["rounds"] == 1
    print("every seed a leader", got["stats"])


@pytest.mark.parametrize("form", [1, 2])
def test_ms3_shift_and_group(cl, form):
    c = clustered(NS, K)
    want = T.clustered_forms(c, 3)
    got = ms_run(cl, c["points"], None, c["radius"], 3, c["tol"], form=form)
    same(got, want, 2)
    assert got["stats"]["passes"] == 2 and got["stats"]["form_used"] == form and got["stats"]["rounds"] == 1
    assert np.array_equal(got["shifted"], c["means"][c["labels"]])      # the cluster mean per seed
    print("shift and group", got["stats"])


def test_ms3_shift_and_group_with_non_finite_rows_behind_the_first_trip(cl):
    c = clustered(NS, K)
    bad = {T.PRIM_TRIP: (0, np.nan), T.PRIM_TRIP + 1: (1, np.inf), T.PRIM_TRIP + 2: (2, -np.inf), 530_000: (2, np.nan), 535_001: (0, -np.inf), NS - 1: (1, np.inf)}
    want = T.clustered_forms(c, 3, bad_rows=bad)
    assert min(bad) >= T.PRIM_TRIP and np.isfinite(want["points"][:T.PRIM_TRIP]).all()
    for device_mem in (False, True):
        got = ms_run(cl, want["points"], None, c["radius"], 3, c["tol"], device_mem=device_mem)
        same(got, want, 3)      # a NaN seed never converges: iterations = max_iter
        assert got["stats"]["passes"] == 2 and np.isnan(got["shifted"][sorted(bad)]).all() and len(got["offsets"]) - 1 == K + 6
        assert (np.diff(got["offsets"])[K:] == 1).all() and np.array_equal(got["members"][got["offsets"][K:-1]], sorted(bad))      # NaN singletons
    print("non-finite rows", got["stats"])


def test_ms3_shift_and_group_with_own_seeds(cl):
    c = clustered(NS, K)
    want = T.clustered_forms(c, 3, reverse_seeds=True)
    got = ms_run(cl, c["points"], want["seeds"], c["radius"], 3, c["tol"])
    same(got, want, 2)
    assert got["stats"]["passes"] == 2
    print("own seeds", got["stats"])


def test_ms3_no_finite_point(cl):
    """n = 0: no grid, the first active list is k_iota's; every ball is empty"""
    seeds = spread(NS_ND, 3)
    got = ms_run(cl, np.zeros((0, 3), np.float32), seeds, 1.0, 3, 0.25)
    every_seed_its_own_cluster(got, NS_ND)
    assert got["iterations"] == 3 and got["stats"]["passes"] == 1 and np.isnan(got["shifted"]).all() and np.isnan(got["modes"]).all() and got["modes"].shape == (NS_ND, 3)


# ---- mean shift, N-d ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [2, 16])
def test_msn_grouping_alone(cl, dim):
    c = clustered(NS_ND, 300, dim)
    want = T.clustered_forms(c, 0)
    for device_mem in (False, True):
        got = msn_run(cl, np.zeros((3, dim), np.float32), c["points"], 1.0, 0, c["tol"], device_mem=device_mem)
        same(got, want, 0)
        assert got["stats"]["rounds"] == 1 and np.array_equal(got["members"][got["offsets"][:-1]], c["leaders"])
    print("nd grouping", dim, got["stats"])


@pytest.mark.parametrize("dim", [2, 16])
def test_msn_shift(cl, dim):
    """524 300 seeds over 8 data points in two tight clusters: one pass to the mean of one of them, a second that finds every seed converged"""
    c = clustered(NS_ND, 300, dim)
    data, in_a = T.two_sinks(c)
    want = T.sink_forms(c, data, in_a)
    got = msn_run(cl, data, c["points"], T.SINK_RADIUS, 3, c["tol"])
    same(got, want, 2)
    assert got["stats"]["passes"] == 2 and got["stats"]["rounds"] == 1 and np.array_equal(got["members"][got["offsets"][:-1]], want["leaders"])
    print("nd shift", dim, got["stats"])


def test_msn_tolerance_zero(cl):
    """the ungrouped path: labels by k_iota, k_ms_modes<5> over 524 300 clusters"""
    seeds = spread(NS_ND, 5)
    got = msn_run(cl, np.zeros((3, 5), np.float32), seeds, 1.0, 0, 0.0)
    every_seed_its_own_cluster(got, NS_ND)
    assert got["iterations"] == 0 and got["stats"]["rounds"] == 0 and bits(got["shifted"]).tobytes() == bits(seeds).tobytes() and bits(got["modes"]).tobytes() == bits(seeds).tobytes()


def test_msn_modes_past_the_wave_cap(cl):
    """k_ms_modes<2> past 16 384 clusters with real member lists (k_msn_lead streams up to 16 400 leaders per lane here: the slow one)"""
    c = clustered(NS, K, 2, side=128)
    want = T.clustered_forms(c, 0)
    got = msn_run(cl, np.zeros((3, 2), np.float32), c["points"], 1.0, 0, c["tol"])
    same(got, want, 0)
    assert got["stats"]["rounds"] == 1 and got["modes"].shape == (K, 2)
    print("nd modes", got["stats"])


# ---- connected components, N-d ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,axis", [(2, 1), (16, 0)])
def test_ccn_chain(dim, axis):
    """600 001 points, four gaps: five segments of different sizes, in form 2 and in form 0 (which is form 2 at this size).  Form 1 would test
    1.8 10^11 pairs here and is left out; its kernels take no capped grid."""
    p, want, sizes = T.chain_nd(600_001, dim, axis, (50_000, 170_000, 300_000, 599_000))
    assert sizes == [50_001, 120_000, 130_000, 299_000, 1000] and np.diff(want[1]).tolist() == sorted(sizes, reverse=True)
    runs = []
    for form in (2, 0, 2):
        st = {}
        got = ccn_run(p, np.float32(1.0), None, form, stats=st)
        for k, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (form, ("labels", "offsets", "members")[k], int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))
        assert st["form_used"] == 2 and st["axis"] == axis
        runs.append(got)
    print("ccn", dim, st)
    for a, b in zip(runs[0], runs[2]):      # two runs agree word for word
        assert a.tobytes() == b.tobytes()


# ---- convex hull --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hull_case(dim):
    pts, meta = T.hull_late(dim)
    return pts, meta, RH.ref_hull(pts)


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("dim", [3, 2])
def test_hull_late(dim, mem):
    pts, meta, ref = hull_case(dim)
    got, info = capi_hull(pts, True, mem)
    hull_check(got, ref, pts)      # vertices, facets, halfspaces bit for bit, the non-finite count, containment within the band
    late = meta["first_late"]
    v = got["vertex_point_indices"].astype(np.int64)
    assert got["n_nonfinite"] == info["n_nonfinite"] == 5
    assert v[0] == 7 and (v[1:] >= late).all() and meta["tie_source"] not in v      # the tie goes to the lowest index, in the first trip
    assert np.array_equal(bits(got["halfspaces"]), bits(ref["halfspaces"]))
    # the seeds of the second trip make a first polytope that holds the whole inner ball: only late finite rows can survive round one
    assert info["survivors_first_round"] <= meta["shell"] + 3 and info["rounds"] >= 2
    print("hull", dim, mem, info)
