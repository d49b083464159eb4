"""Every accumulating kernel's 48 raw f64 sums, BIT FOR BIT, on exact lattices (tests/_sums_refs.py).

On dyadic-lattice data every f32 operation of a per-pair term and every f64 product and sum is exact, so each of the 48 sums of an ICP
iteration (solve.hpp:20-29) is one number whatever the kernel, its order of additions, its wave layout or its block count.  Every
comparison below is np.array_equal against integer arithmetic; there is no tolerance in this module.  tests/test_sums_refs_cpu.py shows
that the fixtures meet the conditions (and pins the restatement to the CPU oracle); here the means the estimators centre with are the
fixture's dyadic ones, handed over with set_shard_info / icp_begin(global_src_mean) and read back through means().

A. the raw sums through icp_begin -> icp_partial_sums (partial_sums_core, the seam of the sharded engines), four metrics (Kabsch, plane,
   point, both) x identity and a quarter turn with an integer shift x the masks all / none / about half / all but one / exactly one, at
   sizes 1, 2, a wave, a block, TILE_THREADS, TILE_QUERIES (each -1, 0, +1), the warm-started form's floor 65,536 (+1, +63) and one trip
   of the streaming kernel's grid (524,288) and one past it, for
     per-lane fused kernel (k_iter, accumulate_pair)      fused = 1
     two passes, per-lane search + streaming pass         tiled = 0, tile_accumulation = 0, warm_start = 0
     two passes, tiled search + streaming pass            tiled = 2, tile_accumulation = 0, warm_start = 0
     in-tile accumulation (k_search_tiled<ACC>)           tiled = 2, tile_accumulation = 2, warm_start = 0
     in-tile clean-up (k_search_deferred<ACC>)            the same, sorted under the identity and begun two lattice steps away
     warm-started form (k_warm<ACC, REC>)                 warm_start = 2 (+ tiled = 2, tile_accumulation = 2): call 1 cold, an all-zero
                                                          update after every call (the transform stays T0 bit for bit), call 2 = first
                                                          form (writes records), call 3 = steady form; also over records the TILE wrote
                                                          (and its tile_records = 0 twin) and with the target's {point, normal} records
                                                          built (pair_records) -- see test_raw_sums_warm_started_form for what the
                                                          icp_begin seam needs to reach each of them
   and the single-match masks at 64, 65, 257 points: every query in turn is the only one inside the radius, the sums are that pair's z z^T.
   Each case proves its form: last_run_forms(), last_warm_iterations(), last_run_trace() (k_warm's first / steady form, the tile),
   debug_counters() (deferred queries) and the option state.
   Omitted by the policy, not skipped: the warm-started form below 65,536 source points (warm_capable()).  tiled = 2 forces the tiles at
   every size, so use_tiled() refuses none of the listed ones, and the drift defers queries at every size (36 of 65, 454 of 2,049,
   19,295 of 524,289; at 1 and 2 points the whole tile goes to the clean-up pass).
B. the host entries over a stored set (find_correspondences first): estimate_point_to_point's moments, estimate_combined's AtA / Atb for
   three dyadic weightings, estimate_affine's AtA[144] / Atb[12] / count (centred and not); the symmetric objective with source normals;
   search_direction 1 and 2 (pair lists: on these lattices every directed set is the same set of pairs, ordered by target index);
   dyadic per-pair weights from {0, 0.5, 1, 2} through set_pair_weight_callback, a zero weight inside a full wave included.
C. one iteration of the device-resident loops: cilhip_icp_run(max_iter = 1, conv_tol = 0) returns bit for bit the T, last_ncorr and
   last_delta_norm of a second context that is handed the EXACT expected sums (icp_begin, icp_apply_sums, icp_state) -- both go through
   the epilogue's solve_body (epilogue.hip; no path with another solve was found) -- for the adaptive default, fused_epilogue = 1,
   search_direction 1 and 2, each with and without require_reciprocality (launch_acc_reverse), and the ranked loop with one rank
   (RANK_ROWS fold); _prove_loop says which loop and form each one took.
D. the SECOND iteration of the reverse loops (FIRST_TO_SECOND, BOTH, BOTH reciprocal): cilhip_icp_run(max_iter = 2, conv_tol = 0) on
   sr.two_step_pair, whose first step is exact by construction -- iteration 0 matches the A group alone, all with ONE residual, and
   steps by -U / 16, so iteration 1 works on lattice data again (B, unmatched before, now carries the residuals; twin targets give the
   reverse half of BOTH matches that are no reciprocal duplicates).  The reference context is handed the exact iteration-0 sums
   (icp_begin, icp_apply_sums): it must report one iteration, |A| pairs and THE predicted T1 -- the translation bit for bit; the linear
   part is T0's up to what the f64 solve leaves (asserted below sr.ABSORB, which tests/test_two_step_refs_cpu.py shows the pinned
   transform expression rounds away: T1 S and T1 src_mean, evaluated here from the device's own T1, are the intended dyadic positions bit
   for bit) -- and is then handed the exact iteration-1 sums of the direction: (T2, last_ncorr, last_delta_norm).  Every run of
   3 directions x reverse_warm_start 1 / 0 x 4 metrics x 2 T0 returns those bytes, twice.  reverse_warm_start = 1: iteration 1 is
   k_reverse_warm<ACC> (WaveRank<ACC>; last_reverse_fused_iterations() == 1), = 0: a full reverse search, then launch_acc_reverse
   (== 0); both with run_reverse_loop's other proofs (_prove_loop: nothing listed, no forward form counted, BOTH's forward half cold).
   Target sizes (twins included): one round of 256 at -1 / 0 / +1, 2,048 / 2,049 (reverse_warm_blocks: 1 -> 2 blocks), 4,352 (17 rounds
   dealt to three blocks: 6, 6 and 5) and 16 * 2048 * 256 + 257 (the block count capped at 2,048, 17 rounds in the first block: the in-loop
   flush() with a wave's list at RW_WCAP exactly, the pipeline's `r + gridDim.x < rounds` branch taken 16 times) against 4,096 source
   points.  In the walk over the sorted target, A sites and twins sit in the last round and in lanes 0 and 63 of a wave, and the first
   block's waves reach the in-loop flush() with nothing settled (test_reverse_walk_meets_a_sites_and_twins_at_its_edges, on the grid
   shape asserted here against get_grid_info).
   Settled or listed.  k_reverse_warm settles a target point iff it has a previous match i, m = smin sqrt(safe2[i]) 0.99999 - 2.0002 eps_q
   is positive, 4 e (1 + 1e-5) < m^2 and e < r^2.  Here: the A sites are the only targets matched at iteration 0, and after the exact step
   their e is 0; safe2 (k_self_nn over the source grid) is the smaller of the squared distance to the nearest other source point -- at
   least (1 - 6/16)^2, two sites apart less the largest difference of two offsets -- and (cell - cell / 512)^2 KSHRINK of a grid
   whose cell is cbrt(volume / ns) > 1 for a source on at most 55 % of the sites; eps_q = motion_eps_of(T1, ...) = 6e-7 (|t| +
   sum |L| (|c| + h)) < 6e-7 * 3 * 700 = 1.3e-3.  So m > 0.5 and every A site is SETTLED (accumulated as it streams by, bidir.hip:394);
   B's sites, the twins, F's and the empty sites have no previous match and are LISTED (searched, then accumulated at bidir.hip:349).
   No read-out shows this: the kernel counts neither, and instrumenting it is not this module's business.
   Limit of the design: a settled A pair has residual 0 at iteration 1 (the step removed it).  Its p, q, a, e and n entries are not zero
   and move AtA and the Kabsch moments, so a stale q or another point's normal on a settled lane still changes T2
   (test_second_iteration_sums_notice_a_wrong_pair); an error that only scales a settled pair's residual would not show.
Not covered: feat_warm.hip's three-cloud accumulation; Gauss-Newton steps after the first (max_optimization_iterations > 1); per-pair
weight callbacks in the reverse loops (they keep the separate pass by design); duplicated source points (the reverse search meets a tie
and the loop leaves the list-free path); BOTH's warm-started forward half (three iterations and >= 65,536 source points); and the Kabsch
moments streamed over a pair list (no host entry reads them, see test_stored_set_host_entries).
"""
import ctypes as C
import time

import numpy as np
import pytest

import _filter_refs as fr
import _sums_refs as sr
from cilantro_amd import capi
from test_gpu_loop_matches import _report

pytestmark = pytest.mark.gpu

FUSED = ("lane fused", (("fused", 1),))
TWO_PASS_LANE = ("two pass, per-lane search", (("tiled", 0), ("tile_accumulation", 0), ("warm_start", 0)))
TWO_PASS_TILED = ("two pass, tiled search", (("tiled", 2), ("tile_accumulation", 0), ("warm_start", 0)))
IN_TILE = ("in-tile", (("tiled", 2), ("tile_accumulation", 2), ("warm_start", 0)))
COLD_FORMS = (FUSED, TWO_PASS_LANE, TWO_PASS_TILED, IN_TILE)
_WARM = (("tiled", 2), ("tile_accumulation", 2), ("warm_start", 2))
_WARM_LATER = (("tiled", 2), ("tile_accumulation", 2), ("warm_start", 1))      # (1: the second call is still the tile; 2 is set before the third)
SEARCH, TILE, WARM_FIRST, WARM = 0, 1, 2, 3      # loop_policy.hpp's FORM_*, as last_run_trace() names an iteration's form
# (name, options, a Gauss-Newton icp_run first (it builds the target's {point, normal} records), warm_start = 2 before the last call, forms)
WARM_FORMS = (("warm", _WARM, False, False, (TILE, WARM_FIRST, WARM)),
              ("warm, pair records", _WARM, True, False, (TILE, WARM_FIRST, WARM)),
              ("warm after a record-writing tile", _WARM_LATER, False, True, (TILE, TILE, WARM)),
              ("warm after a tile, tile_records 0", _WARM_LATER + (("tile_records", 0),), False, True, (TILE, TILE, WARM_FIRST)),
              ("two pass, pair records", TWO_PASS_TILED[1], True, False, (SEARCH,)))
CLEANUP_SIZES = sr.SIZES                                 # (the drift defers queries at every size; at 1 and 2 points the whole tile)
DRIFT = (2, -1, 1)                                       # lattice steps between the sort and the search
PARAMS = {sr.KABSCH: (capi.METRIC_POINT_TO_POINT, 0.0, 1.0), sr.PLANE: (capi.METRIC_COMBINED, 0.0, 1.0),
          sr.POINT: (capi.METRIC_COMBINED, 1.0, 0.0), sr.BOTH: (capi.METRIC_COMBINED, 0.5, 0.25)}
_figures = {}
_expected = {}


@pytest.fixture(scope="module")
def Context(hip_lib):
    from cilantro_amd.icp import Context as Ctx

    return Ctx


@pytest.fixture(scope="module")
def dev(hip_lib):
    import torch

    class Dev:
        stream = torch.cuda.current_stream().cuda_stream
        buf = torch.zeros(capi.SUMS_LEN, dtype=torch.float64, device="cuda")

        @staticmethod
        def read():
            return Dev.buf.cpu().numpy().copy()

        @staticmethod
        def write(v):
            Dev.buf.copy_(torch.from_numpy(np.ascontiguousarray(v, np.float64)))

    return Dev


@pytest.fixture(scope="module", autouse=True)
def _figures_report():
    """the counts per form and size, next to the run"""
    yield
    if _figures:
        _report("exact_sums_cases.json", _figures)


def expected(n, metric, mask):
    """the exact sums of (size, metric, mask): computed once, shared by every form, transform and section (they do not depend on T)"""
    key = (n, metric, mask)
    if key not in _expected:
        fix = sr.fixture(n)
        _expected[key] = sr.expected_sums_of(fix, metric, sr.masks(fix)[mask][1])[1]
    return _expected[key]


def _open(Context, dev, fix, options):
    ctx = Context(0, dev.stream)
    for k, v in options:
        ctx.set_option(k, v)
    ctx.set_target(fix["D"], fix["N"])
    for k, v in options:
        assert ctx.get_option(k) == v
    return ctx


def _load(ctx, fix, S=None):
    """the source (as stored under the fixture's transform) and the dyadic means"""
    ctx.set_source(fix["S"] if S is None else S, fix.get("SN"))
    ctx.set_shard_info(0, dst_mean=fix["dst_mean"], src_mean=fix["src_mean"])
    dm, sm = ctx.means()
    assert np.array_equal(dm, fix["dst_mean"]) and np.array_equal(sm, fix["src_mean"])


def _params(ctx, metric, r2, max_iter=100):
    p = capi.IcpParams()
    ctx._L.cilhip_icp_default_params(C.byref(p))
    p.metric, p.w_p2p, p.w_p2pl = PARAMS[metric]
    p.max_sq_dist, p.max_iter, p.conv_tol, p.max_opt_iter = float(r2), max_iter, 0.0, 1
    return p


def _partial_sums(ctx, dev):
    ctx.icp_partial_sums(dev.buf.data_ptr())
    return dev.read()


def _prove_cold(ctx, name):
    one, two = ctx.last_run_forms()
    warm = ctx.last_warm_iterations()
    want = {FUSED[0]: (0, 0), TWO_PASS_LANE[0]: (0, 1), TWO_PASS_TILED[0]: (0, 1), IN_TILE[0]: (1, 0)}[name]
    assert (one, two) == want and warm == 0, (name, one, two, warm)


def _T_bits(res):
    return bytes(np.array(res.T[:], np.float32))


def _note(name, obj):
    _figures[name] = obj


# ---- A. the raw sums of every form -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", sr.SIZES)
def test_raw_sums_every_cold_form(Context, dev, n):
    t0 = time.perf_counter()
    cases = {}
    fixes = {t: sr.fixture(n, t) for t in sr.A_TRANSFORMS}
    for name, options in COLD_FORMS:
        ctx = _open(Context, dev, fixes["identity"], options)
        for tname, fix in fixes.items():
            _load(ctx, fix)
            for mask, (r2, has) in sr.masks(fix).items():
                for metric in sr.METRICS:
                    ctx.icp_begin(_params(ctx, metric, r2), fix["T"], fix["src_mean"])
                    got = _partial_sums(ctx, dev)
                    _prove_cold(ctx, name)
                    exp = expected(n, metric, mask)
                    assert exp[0] == has.sum() and (not has.any() or np.all(got[sr.used_slots(metric)] != 0.0))
                    assert np.array_equal(got, exp), (n, name, tname, mask, metric, np.nonzero(got != exp)[0], got[got != exp], exp[got != exp])
                    cases[name] = cases.get(name, 0) + 1
        ctx.close()
    print("exact sums, cold forms", n, cases, "%.2f s" % (time.perf_counter() - t0))
    _note(f"cold/{n}", cases)


@pytest.mark.parametrize("n", sr.WARM_SIZES)
def test_raw_sums_warm_started_form(Context, dev, n):
    """Every call is followed by an all-zero update (Kabsch and Gauss-Newton alike: no pairs = the identity step, the transform stays T0
    bit for bit), so every call sees the same exact problem and last_run_trace() names the form of each: the same expected vector every time.
      warm                               call 1 the cold tile (run_calls = 0: it never writes records, whatever tile_records says), call 2
                                         k_warm's FIRST form (gathers through the stored positions, writes the records), call 3 its steady form
      warm, pair records                 the same after a Gauss-Newton icp_run on the context: from 65,536 source points up that run builds the
                                         target's {point, normal} records (ensure_pair_records, option pair_records = 1), which k_warm's plane
                                         metrics then gather from; the variant above, which never ran one, is the side without them
      warm after a record-writing tile   warm_start = 1 for two calls: call 2 (run_calls = 1) is the accumulating tile again and leaves the
                                         match records itself; warm_start = 2 then makes call 3 k_warm's STEADY form over tile-written records
      ... tile_records 0                 the same with the tile writing none: call 3 is k_warm's FIRST form instead
      two pass, pair records             the streaming pass gathering from the {point, normal} records (one call)
    Nothing reports whether the {point, normal} records exist: what stands for it is the code's condition -- a Gauss-Newton icp_run at
    ns >= 65536 on a target with normals, pair_records = 1 (read back) -- and the run itself being asserted."""
    t0 = time.perf_counter()
    cases = {}
    fixes = {t: sr.fixture(n, t) for t in sr.A_TRANSFORMS}
    for name, options, prime, later, forms in WARM_FORMS:
        ctx = _open(Context, dev, fixes["identity"], options)
        assert ctx.get_option("pair_records") == 1 and ctx.get_option("tile_records") == (0 if ("tile_records", 0) in options else 1)
        want_forms = (sum(f != SEARCH for f in forms), sum(f == SEARCH for f in forms))
        want_warm = sum(f in (WARM_FIRST, WARM) for f in forms)
        for tname, fix in fixes.items():
            _load(ctx, fix)
            if prime:
                res = ctx.icp_run(_params(ctx, sr.BOTH, sr.masks(fix)["all"][0], 1), fix["T"])
                assert int(res.iterations) == 1 and int(res.last_ncorr) == n
            T0_bits = bytes(np.ascontiguousarray(fix["T"].T, np.float32))      # (column-major, as IcpResult holds it)
            for mask, (r2, has) in sr.masks(fix).items():
                for metric in sr.METRICS:
                    exp = expected(n, metric, mask)
                    if later:
                        ctx.set_option("warm_start", 1)
                    ctx.icp_begin(_params(ctx, metric, r2), fix["T"], fix["src_mean"])
                    for call in range(len(forms)):
                        if later and call == len(forms) - 1:
                            ctx.set_option("warm_start", 2)
                        got = _partial_sums(ctx, dev)
                        assert np.array_equal(got, exp), (n, name, tname, mask, metric, call, np.nonzero(got != exp)[0], got[got != exp], exp[got != exp])
                        dev.write(np.zeros(capi.SUMS_LEN))
                        ctx.icp_apply_sums(dev.buf.data_ptr())
                        st = ctx.icp_state()
                        assert _T_bits(st) == T0_bits and int(st.iterations) == call + 1 and int(st.last_ncorr) == 0, (n, name, tname, metric, call)
                    ran = tuple(t["form"] for t in ctx.last_run_trace())
                    assert ran == forms and ctx.last_run_forms() == want_forms and ctx.last_warm_iterations() == want_warm, (n, name, tname, mask, metric, ran)
                    cases[name] = cases.get(name, 0) + len(forms)
        ctx.close()
    print("exact sums, warm-started form", n, cases, "%.2f s" % (time.perf_counter() - t0))
    _note(f"warm/{n}", cases)


@pytest.mark.parametrize("n", CLEANUP_SIZES)
def test_raw_sums_in_tile_cleanup_pass(Context, dev, n):
    """the source sorted under the identity, the search begun DRIFT lattice steps away: queries leave their tiles' reach and go through
    k_search_deferred<ACC> -- debug_counters() must show them"""
    fix = sr.fixture(n)
    T0 = np.eye(4, dtype=np.float32)
    T0[:3, 3] = DRIFT
    S = np.ascontiguousarray(fix["S"] - T0[:3, 3])
    assert np.array_equal(S.astype(np.float64), fix["S"].astype(np.float64) - np.array(DRIFT, np.float64))
    src_mean = fix["src_mean"] - T0[:3, 3]
    assert np.array_equal(sr.transform_points(T0, S, np.float32), fix["q"])
    ctx = _open(Context, dev, fix, IN_TILE[1])
    ctx.set_source(S)
    ctx.set_shard_info(0, dst_mean=fix["dst_mean"], src_mean=src_mean)
    ctx.find_correspondences(np.eye(4, dtype=np.float32), 0.25, count=False)      # the sort happens here, under the identity
    cases = 0
    deferred = {}
    for mask, (r2, has) in sr.masks(fix).items():
        for metric in sr.METRICS:
            ctx.icp_begin(_params(ctx, metric, r2), T0, src_mean)
            got = _partial_sums(ctx, dev)
            _prove_cold(ctx, IN_TILE[0])
            dq, dt = ctx.debug_counters()
            assert dq + dt > 0, (n, mask, metric, dq, dt)
            deferred[mask] = (dq, dt)
            exp = expected(n, metric, mask)
            assert np.array_equal(got, exp), (n, mask, metric, np.nonzero(got != exp)[0], got[got != exp], exp[got != exp])
            cases += 1
    ctx.close()
    print("exact sums, in-tile clean-up pass", n, cases, deferred)
    _note(f"cleanup/{n}", {"cases": cases, "deferred (queries, tiles)": deferred})


@pytest.mark.parametrize("n", sr.SINGLE_SIZES)
def test_single_match_walks_every_lane(Context, dev, n):
    """query k alone inside the radius, for every k (even k under the identity, odd k under the quarter turn): the 48 sums are that one
    pair's -- every lane of a wave and the first of the next, whatever the sort order made of the indices"""
    t0 = time.perf_counter()
    fixes = [sr.fixture(n, t) for t in sr.A_TRANSFORMS]
    ctxs = [(name, _open(Context, dev, fixes[0], options)) for name, options in (FUSED, TWO_PASS_LANE, IN_TILE)]
    cases = 0
    for k in range(n):
        g = sr.single_match_fixture(n, k)
        r2, has = sr.masks(g)["one"]
        assert has.sum() == 1 and has[k]
        exp = {m: sr.expected_sums_of(g, m, has)[1] for m in sr.METRICS}
        for name, ctx in ctxs:
            _load(ctx, g)
            for metric in sr.METRICS:
                ctx.icp_begin(_params(ctx, metric, r2), g["T"], g["src_mean"])
                got = _partial_sums(ctx, dev)
                assert got[0] == 1.0 and np.array_equal(got, exp[metric]), (n, k, name, metric, np.nonzero(got != exp[metric])[0])
                cases += 1
            _prove_cold(ctx, name)
    for _name, ctx in ctxs:
        ctx.close()
    print("exact sums, single match", n, cases, "%.2f s" % (time.perf_counter() - t0))
    _note(f"single/{n}", cases)


# ---- B. the host entries over a stored set ---------------------------------------------------------------------------------------------

def _estimate_affine(ctx, w_p2p, w_p2pl, centered):
    """cilhip_estimate_affine with its count (Context.estimate_affine hands back AtA, Atb and `ok`, not how many pairs went in)"""
    T = np.zeros(16, np.float32); AtA = np.zeros(144, np.float64); Atb = np.zeros(12, np.float64)
    ok = C.c_int(0); n = C.c_size_t(0)
    ctx._ck(ctx._L.cilhip_estimate_affine(ctx._h, w_p2p, w_p2pl, 1 if centered else 0, T.ctypes.data, AtA.ctypes.data, Atb.ctypes.data, C.byref(n), C.byref(ok)))
    return AtA.reshape(12, 12), Atb, int(n.value)


def _cached(key, make):
    """(nothing expected depends on the transform or the search direction: q, the means under T and the set of pairs are the same)"""
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def _half(fix):
    m = sr.masks(fix)
    return m["half"] if "half" in m else m["all"]


@pytest.mark.parametrize("n", sr.STORED_SIZES)
def test_stored_set_host_entries(Context, dev, n):
    """estimate_point_to_point runs for SECOND_TO_FIRST alone: the entry needs the per-query matches (have_nn) and refuses a pair list
    (estimate.hip), so the Kabsch moments streamed over a PAIR LIST have no host entry to be read through and are not covered here;
    estimate_combined and estimate_affine take every direction's set."""
    cases = 0
    for tname in ("identity", "rz90_shift", "mirror_z"):
        fix = sr.fixture(n, tname)
        r2, has = _half(fix)
        mask = "half" if "half" in sr.masks(fix) else "all"
        ctx = _open(Context, dev, fix, ())
        _load(ctx, fix)
        for direction in (0, 1, 2):
            ctx.set_option("search_direction", direction)
            assert ctx.find_correspondences(fix["T"], float(r2)) == has.sum()
            # the stored set is the lattice's by construction: forward ascending by source index; FIRST_TO_SECOND the reverse set, BOTH
            # its union with the forward one (tests/_filter_refs.py), both ordered by (target, source) index
            si = np.nonzero(has)[0]
            fwd = (fix["match"][si], si, fix["d2"][si])
            o = np.argsort(fwd[0], kind="stable")
            rev = tuple(x[o] for x in fwd)
            want = fwd if direction == 0 else (rev if direction == 1 else fr.union(rev, fwd))
            assert fr.same(ctx.get_correspondences(), want), (n, tname, direction)
            if direction == 0:
                _T, sums, _ok = ctx.estimate_point_to_point()
                assert np.array_equal(sums, expected(n, sr.KABSCH, mask)[:16]), (n, tname, "kabsch")
                cases += 1
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                _T, AtA, Atb, _cv = ctx.estimate_combined(w_p2p, w_p2pl, 1, 0.0)
                eA, eb = sr.gn_normal_equations(expected(n, sr.metric_of_weights(w_p2p, w_p2pl), mask), w_p2p, w_p2pl)
                assert np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, direction, w_p2p, w_p2pl)
                cases += 1
                for centered in (False, True):
                    AtA, Atb, cnt = _estimate_affine(ctx, w_p2p, w_p2pl, centered)
                    eA, eb, ecnt = _cached(("affine", n, w_p2p, w_p2pl, centered), lambda: sr.expected_affine(fix, has, w_p2p, w_p2pl, centered))
                    assert cnt == ecnt and np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, direction, w_p2p, w_p2pl, centered)
                    cases += 1
        # per-pair weights from the callback, by source index; the metric weights multiply them in f32 (exact: dyadic)
        ctx.set_option("search_direction", 0)
        wq, wp = sr.pair_weights(fix, has)
        calls = []

        def weigh(i1, i2, val):
            calls.append((i1.copy(), i2.copy(), val.copy()))      # (looked at after the estimates, outside the foreign call)
            return wq[i2], wp[i2]

        ctx.set_pair_weight_callback(weigh)
        for direction in (0, 2):
            ctx.set_option("search_direction", direction)
            ctx.find_correspondences(fix["T"], float(r2))
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                _T, AtA, Atb, _cv = ctx.estimate_combined(w_p2p, w_p2pl, 1, 0.0)
                metric = sr.metric_of_weights(w_p2p, w_p2pl)
                es = _cached(("weighted", n, w_p2p, w_p2pl), lambda: sr.expected_sums_of(fix, metric, has, weights=(np.float32(w_p2p) * wq, np.float32(w_p2pl) * wp))[1])
                eA, eb = sr.gn_normal_equations(es, 1.0 if w_p2p > 0 else 0.0, 1.0 if w_p2pl > 0 else 0.0, point_weighted=True)
                assert np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, direction, "weighted", w_p2p, w_p2pl)
                cases += 1
        assert calls
        for i1, i2, val in calls:
            assert len(i2) == has.sum() and np.array_equal(i1, fix["match"][i2]) and np.array_equal(val, fix["d2"][i2]), (n, tname)
        ctx.set_pair_weight_callback(None)
        ctx.close()
    # the symmetric objective: source normals set, n = n_dst + T.linear() n_src
    for tname in ("identity", "rz90_shift"):
        fix = sr.fixture(n, tname, "symmetric")
        r2, has = _half(fix)
        ctx = _open(Context, dev, fix, ())
        _load(ctx, fix)
        assert ctx.get_option("symmetric_metric") == 1
        for direction in (0, 1, 2):
            ctx.set_option("search_direction", direction)
            assert ctx.find_correspondences(fix["T"], float(r2)) == has.sum()
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                _T, AtA, Atb, _cv = ctx.estimate_combined(w_p2p, w_p2pl, 1, 0.0)
                eA, eb = sr.gn_normal_equations(sr.expected_sums_of(fix, sr.metric_of_weights(w_p2p, w_p2pl), has)[1], w_p2p, w_p2pl)
                assert np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, "symmetric", direction, w_p2p, w_p2pl)
                cases += 1
        ctx.close()
    print("exact sums, stored-set entries", n, cases)
    _note(f"stored/{n}", cases)


# ---- C. one iteration of the device-resident loops -------------------------------------------------------------------------------------

FORWARD, REVERSE, RANKED = "forward", "reverse", "ranked"
LOOPS = (("adaptive", (), FORWARD), ("fused_epilogue", (("fused_epilogue", 1),), FORWARD),
         ("first_to_second", (("search_direction", 1),), REVERSE),
         ("first_to_second, reciprocal", (("search_direction", 1), ("require_reciprocality", 1)), REVERSE),
         ("both", (("search_direction", 2),), REVERSE),
         ("both, reciprocal", (("search_direction", 2), ("require_reciprocality", 1)), REVERSE), ("ranked, one rank", (), RANKED))
# the form the default policy gives the one iteration at these sizes: below 600 tiles use_tiled() keeps the per-lane search, so the sums
# come from the streaming pass (last_run_forms() == (0, 1))
DEFAULT_FORM = {257: SEARCH, 2049: SEARCH, 65537: SEARCH}


def _prove_loop(ctx, kind, n):
    """which loop and which form the one iteration took.  forward / ranked: the form of DEFAULT_FORM, by last_run_trace() and
    last_run_forms().  reverse (search_direction 1 / 2): run_other_directions' list-free conditions hold here (no post-filter, no source
    normals, a rigid T0, both clouds non-empty, no feature weights, no tie met by a reverse search: the lattices have none), so run_reverse_loop
    (launch_acc_reverse) runs and not the pair-list loop: it lists nothing (last_matches_origin() == 2, searched again on demand; the
    pair-list loop leaves its list: 1) and counts no forward form."""
    forms, warm = ctx.last_run_forms(), ctx.last_warm_iterations()
    if kind == REVERSE:
        assert ctx.last_matches_origin() == 2 and forms == (0, 0) and warm == 0, (n, kind, ctx.last_matches_origin(), forms, warm)
        return "reverse loop"
    ran = tuple(t["form"] for t in ctx.last_run_trace())
    want = DEFAULT_FORM[n]
    assert ran == (want,) and forms == ((0, 1) if want == SEARCH else (1, 0)) and warm == 0, (n, kind, ran, forms, warm)
    if kind == FORWARD:
        assert ctx.last_matches_origin() == 1, (n, kind, ctx.last_matches_origin())      # (the loop's kernels left the matches)
    return "form %d" % want


@pytest.mark.parametrize("n", sr.LOOP_SIZES)
def test_one_loop_iteration_is_the_solve_of_the_exact_sums(Context, dev, n):
    cases = {}
    proof = {}
    for tname in sr.A_TRANSFORMS:
        fix = sr.fixture(n, tname)
        ref = _open(Context, dev, fix, ())
        _load(ref, fix)
        want = {}
        for mask in ("half", "all"):
            r2, has = sr.masks(fix)[mask]
            for metric in sr.METRICS:
                ref.icp_begin(_params(ref, metric, r2, 1), fix["T"], fix["src_mean"])
                dev.write(expected(n, metric, mask))
                ref.icp_apply_sums(dev.buf.data_ptr())
                st = ref.icp_state()
                assert int(st.iterations) == 1 and int(st.last_ncorr) == has.sum()
                want[(mask, metric)] = (_T_bits(st), int(st.last_ncorr), np.float32(st.last_delta_norm).tobytes())
        ref.close()
        for name, options, kind in LOOPS:
            ctx = _open(Context, dev, fix, options)
            _load(ctx, fix)
            if kind == RANKED:
                ctx.rank_comm_init(Context.rank_comm_unique_id(), 1, 0)
            for mask in ("half", "all"):
                r2, has = sr.masks(fix)[mask]
                for metric in sr.METRICS:
                    p = _params(ctx, metric, r2, 1)
                    if kind == RANKED:
                        ctx.icp_begin(p, fix["T"], fix["src_mean"])
                        ctx.icp_iterate_ranked(1)
                        res = ctx.icp_state()
                    else:
                        res = ctx.icp_run(p, fix["T"])
                    assert int(res.iterations) == 1
                    proof[name] = _prove_loop(ctx, kind, n)
                    got = (_T_bits(res), int(res.last_ncorr), np.float32(res.last_delta_norm).tobytes())
                    assert got == want[(mask, metric)], (n, tname, name, mask, metric, got[1], want[(mask, metric)][1])
                    cases[name] = cases.get(name, 0) + 1
            if kind == RANKED:
                ctx.rank_comm_destroy()
            ctx.close()
    print("exact sums, one loop iteration", n, cases, proof)
    _note(f"loop/{n}", {"cases": cases, "ran": proof})


# ---- D. the second iteration of the reverse loops, after an exact step -----------------------------------------------------------------

REVERSE_DIRECTIONS = (("first_to_second", (("search_direction", 1), ("require_reciprocality", 0))),
                      ("both", (("search_direction", 2), ("require_reciprocality", 0))),
                      ("both_reciprocal", (("search_direction", 2), ("require_reciprocality", 1))))


def _result(res):
    return _T_bits(res), int(res.last_ncorr), np.float32(res.last_delta_norm).tobytes()


def _assert_first_step(st, fix, where):
    """the state after the exact iteration-0 sums: one iteration over the A pairs, the predicted T1 -> (whether T's bits ARE T1's, the
    largest deviation of the linear part from T0's)"""
    na = len(fix["pairs0"][0])
    assert int(st.iterations) == 1 and int(st.last_ncorr) == na, (where, int(st.iterations), int(st.last_ncorr), na)
    T1 = np.array(st.T[:], np.float32).reshape(4, 4).T.copy()      # (IcpResult holds it column-major)
    noise = float(np.abs(T1[:3, :3].astype(np.float64) - fix["T"][:3, :3].astype(np.float64)).max())
    assert np.array_equal(T1[:3, 3], fix["T1"][:3, 3]) and np.array_equal(T1[3], np.array([0, 0, 0, 1], np.float32)), (where, T1, fix["T1"])
    assert noise <= sr.ABSORB, (where, noise)
    assert np.array_equal(sr.transform_points(T1, fix["S"], np.float32), fix["q1"]), (where, noise)
    assert np.array_equal(sr.transform_points(T1, fix["src_mean"].reshape(1, 3), np.float32)[0], fix["smt1"]), (where, noise)
    return bool(np.array_equal(T1, fix["T1"])), noise


@pytest.mark.parametrize("nd", sr.TWO_STEP_SIZES)
def test_second_loop_iteration_is_the_solve_of_the_exact_sums(Context, dev, nd):
    t_all = time.perf_counter()
    assert {m: PARAMS[m][1:] for m in sr.METRIC_WEIGHTS} == sr.METRIC_WEIGHTS
    cases, proof, exact_T1, noise_max = {}, {}, 0, 0.0
    run_s = []
    fix0 = sr.two_step_pair(nd, sr.A_TRANSFORMS[0])
    t_fix = time.perf_counter() - t_all
    ref = _open(Context, dev, fix0, ())
    ctx = _open(Context, dev, fix0, ())
    # the order the reverse kernels walk the target in: the restated grid (sr.grid_order) is the library's
    gi, shape = ctx.grid_info(), sr.grid_order(fix0["D"], order=False)
    assert (gi.nx, gi.ny, gi.nz) == (shape["nx"], shape["ny"], shape["nz"]) and float(gi.cell) == shape["cell"], (nd, gi.nx, gi.ny, gi.nz, gi.cell, shape)
    assert [float(v) for v in gi.origin] == shape["origin"], (nd, list(gi.origin), shape)
    for tname in sr.A_TRANSFORMS:
        fix = sr.two_step_pair(nd, tname)
        assert fix["D"] is fix0["D"]
        _load(ref, fix)
        _load(ctx, fix)
        r2 = fix["r2"]
        want = {}
        for metric in sr.METRICS:
            exp0 = sr.expected_sums_pairs(fix, metric, fix["T"], fix["pairs0"])[1]
            exp1 = {}
            for d, _opts in REVERSE_DIRECTIONS:
                if d == "both":
                    exp1[d] = exp1["first_to_second"]      # (the same pairs by design: forward A + B and the twins)
                    assert all(np.array_equal(x, y) for x, y in zip(fix["pairs1"][d], fix["pairs1"]["first_to_second"]))
                else:
                    exp1[d] = sr.expected_sums_pairs(fix, metric, fix["T1"], fix["pairs1"][d])[1]
                ref.icp_begin(_params(ref, metric, r2, 2), fix["T"], fix["src_mean"])
                dev.write(exp0)
                ref.icp_apply_sums(dev.buf.data_ptr())
                exact, noise = _assert_first_step(ref.icp_state(), fix, (nd, tname, metric))
                exact_T1 += exact
                noise_max = max(noise_max, noise)
                dev.write(exp1[d])
                ref.icp_apply_sums(dev.buf.data_ptr())
                st = ref.icp_state()
                assert int(st.iterations) == 2 and int(st.last_ncorr) == len(fix["pairs1"][d][0]) and float(st.last_delta_norm) > 0.0
                want[(metric, d)] = _result(st)
            assert want[(metric, "both")] == want[(metric, "first_to_second")] != want[(metric, "both_reciprocal")]
        for d, opts in REVERSE_DIRECTIONS:
            for k, v in opts:
                ctx.set_option(k, v)
            for rws in (1, 0):
                ctx.set_option("reverse_warm_start", rws)
                assert all(ctx.get_option(k) == v for k, v in opts) and ctx.get_option("reverse_warm_start") == rws
                name = "%s, reverse_warm_start %d" % (d, rws)
                for metric in sr.METRICS:
                    p = _params(ctx, metric, r2, 2)
                    got = []
                    for _again in range(2):
                        t0 = time.perf_counter()
                        res = ctx.icp_run(p, fix["T"])
                        run_s.append(time.perf_counter() - t0)
                        assert int(res.iterations) == 2
                        _prove_loop(ctx, REVERSE, nd)      # (the list-free reverse loop; BOTH's forward half cold)
                        fused = ctx.last_reverse_fused_iterations()
                        assert fused == rws, (nd, tname, name, metric, fused)      # (iteration 1: k_reverse_warm<ACC> | search + launch_acc_reverse)
                        got.append(_result(res))
                    assert got[0] == want[(metric, d)], (nd, tname, name, metric, got[0][1], want[(metric, d)][1])
                    assert got[1] == got[0], (nd, tname, name, metric, "a repeated run differs")
                    cases[name] = cases.get(name, 0) + 1
                proof[name] = "reverse loop, iteration 1 " + ("in k_reverse_warm" if rws else "search + launch_acc_reverse")
    ref.close()
    ctx.close()
    wall = time.perf_counter() - t_all
    print("exact sums, second loop iteration", nd, cases, "T1 bit-exact in %d of %d reference steps, linear part within %.3g" % (exact_T1, 24, noise_max),
          "%.2f s (fixture %.2f s, slowest run %.4f s)" % (wall, t_fix, max(run_s)))
    _note(f"second/{nd}", {"cases": cases, "ran": proof, "source points": int(fix0["n"]), "pairs, iteration 0": len(fix0["pairs0"][0]),
                           "pairs, iteration 1": {d: len(fix0["pairs1"][d][0]) for d, _o in REVERSE_DIRECTIONS},
                           "reference steps with T1 bit-exact": exact_T1, "largest deviation of T1's linear part": noise_max,
                           "wall s": round(wall, 3), "fixture s": round(t_fix, 3), "runs": len(run_s), "slowest run s": round(max(run_s), 5),
                           "runs total s": round(sum(run_s), 4)})
