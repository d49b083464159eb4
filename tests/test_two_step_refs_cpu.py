"""No GPU: the two-iteration fixture of tests/_sums_refs.py (two_step_pair) held to the conditions section D of
tests/test_gpu_exact_sums.py rests on, for every size and T0 that section runs:
  * the data is exact under T0 and under the predicted T1 (f32 == f64 evaluation of every term, entries multiples of 2^-5, every sum
    inside 53 bits);
  * a search in f64, both directions, both iterations, finds the designed sets, no nearest neighbour tied, no distance at the radius;
  * the step: the exact iteration-0 sums, solved in f64 and composed as the epilogue does, land on T1 -- the translation's f32 image IS
    the predicted one and the transformed source IS the intended dyadic positions, bit for bit, also with every entry of the linear
    part pushed ABSORB off (the round-off a solve leaves, printed, is three orders of magnitude below that);
  * the iteration-1 restatement over the pair lists is the CPU oracle's, bit for bit;
  * it notices a dropped or doubled pair of every group, and the walk of the reverse kernels over the sorted target meets A sites and
    twins in its last round and in the first and last lane of a wave."""
import numpy as np
import pytest

import _sums_refs as sr

SIZES = sr.TWO_STEP_SIZES
DENSE = tuple(n for n in SIZES if n <= 4352)
TNAMES = sr.A_TRANSFORMS


def _ss(v):
    return int((np.asarray(v, np.int64) ** 2).sum())


def test_offsets_meet_the_design():
    u, f, w = sr.TWO_STEP_U, sr.TWO_STEP_F, sr.TWO_STEP_W
    assert _ss(u) < 10 and _ss(f) >= 11 and _ss(f - u) >= 11 and _ss(w - u) >= 11 and 0 < _ss(w) <= 10
    assert len({tuple(d) for d in sr.TWO_STEP_DELTAS}) >= 3
    for d in sr.TWO_STEP_DELTAS:
        assert _ss(u + d) >= 11 and 0 < _ss(d) <= 10
    r2 = float(sr.two_step_pair(SIZES[0])["r2"])
    assert 10.0 / 256.0 < r2 < 11.0 / 256.0 and float(np.float32(r2)) == r2
    # nothing moves further than 1/4 from its site in either iteration: nearest_by_site's premise
    assert max(np.abs(u + d).max() for d in sr.TWO_STEP_DELTAS) <= 4 and np.abs(f - u).max() <= 4 and np.abs(w).max() <= 4
    assert sr.TWO_STEP_LARGE >= 16 * 2048 * 256 + 257


@pytest.mark.parametrize("nd", SIZES)
def test_fixture_is_exact_under_T0_and_T1(nd):
    for tname in TNAMES:
        fix = sr.two_step_pair(nd, tname)
        assert fix["D"].dtype == np.float32 and fix["S"].dtype == np.float32 and len(fix["D"]) == nd and nd > fix["n"]
        assert np.abs(fix["D"]).min() >= 2.0 and np.abs(fix["S"]).min() >= 2.0      # (what ABSORB's bound stands on)
        assert np.abs(fix["D"]).sum(1).max() < 2048.0 and np.abs(fix["S"]).sum(1).max() < 2048.0
        na = int((fix["group"] == sr.GROUP_A).sum())
        assert na >= 16 and len(fix["pairs0"][0]) == na and len(fix["tw_t"]) >= 8
        assert np.array_equal(fix["T1"][:3, :3], fix["T"][:3, :3])
        assert np.array_equal(fix["T1"][:3, 3].astype(np.float64), fix["T"][:3, 3].astype(np.float64) - sr.TWO_STEP_U / 16.0)
        for metric in sr.METRICS:
            num0, _ = sr.assert_exact_pairs(fix, metric, fix["T"], fix["q0"], fix["smt0"], fix["pairs0"])
            assert all(num0[s] != 0 for s in sr.used_slots(metric)), (nd, tname, metric)
            nums = {}
            for d in sr.TWO_STEP_DIRECTIONS:
                nums[d], _ = sr.assert_exact_pairs(fix, metric, fix["T1"], fix["q1"], fix["smt1"], fix["pairs1"][d])
                # after the step the A pairs have no residual; B's and the twins' keep every slot occupied and apart
                assert sr._distinct_nonzero(metric, nums[d]), (nd, tname, metric, d)
            assert nums["first_to_second"] == nums["both"] != nums["both_reciprocal"] and nums["both_reciprocal"] != num0


@pytest.mark.parametrize("nd", SIZES)
def test_f64_searches_find_the_designed_sets(nd):
    fix = sr.two_step_pair(nd, TNAMES[0])
    for tname in TNAMES[1:]:      # (the transformed source is the same cloud under every T0: one search serves them all)
        other = sr.two_step_pair(nd, tname)
        assert np.array_equal(other["q0"], fix["q0"]) and np.array_equal(other["q1"], fix["q1"]) and other["D"] is fix["D"]
        assert all(np.array_equal(a, b) for d in sr.TWO_STEP_DIRECTIONS for a, b in zip(other["pairs1"][d], fix["pairs1"][d]))
    a = np.nonzero(fix["group"] == sr.GROUP_A)[0]
    ab = np.nonzero(fix["group"] != sr.GROUP_F)[0]
    for it, q in enumerate((fix["q0"], fix["q1"])):
        got = sr.loop_sets(fix, q, fix["r2"])      # (asserts: no tie, nothing at the radius)
        for d in sr.TWO_STEP_DIRECTIONS:
            want = sr._pair_set(fix["pairs0"] if it == 0 else fix["pairs1"][d])
            assert got[d] == want, (nd, it, d, len(got[d]), len(want))
        fwd = a if it == 0 else ab
        assert got["forward"] == sr._pair_set((fix["site_t"][fwd], fwd))
        if it == 1:      # BOTH: what the reverse half adds to the forward one is the twins, all of them and nothing else
            assert got["both"] - got["forward"] == sr._pair_set((fix["tw_t"], fix["tw_s"]))


@pytest.mark.parametrize("nd", DENSE)
def test_site_search_is_the_full_distance_matrix(nd):
    fix = sr.two_step_pair(nd, "rz90_shift")
    D64 = fix["D"].astype(np.float64)
    for q in (fix["q0"], fix["q1"]):
        q64 = q.astype(np.float64)
        dd = ((q64[:, None, :] - D64[None, :, :]) ** 2).sum(2)
        for X, Y, M in ((q64, D64, dd), (D64, q64, dd.T)):
            idx, d1, d2 = sr.nearest_by_site(X, Y)
            o = np.argsort(M, 1)[:, :2]
            m1 = np.take_along_axis(M, o[:, :1], 1)[:, 0]; m2 = np.take_along_axis(M, o[:, 1:2], 1)[:, 0]
            near = m1 < 0.25
            assert np.array_equal(idx[near], o[near, 0]) and np.array_equal(d1[near], m1[near]) and np.all(d1[~near] >= 0.25)
            assert np.all(np.minimum(d2[near], 1.0) == np.minimum(m2[near], 1.0))


@pytest.mark.parametrize("nd", SIZES)
def test_first_step_lands_on_T1(nd):
    rng = np.random.default_rng(nd)
    worst = {}
    for tname in TNAMES:
        fix = sr.two_step_pair(nd, tname)
        for metric in sr.METRICS:
            sums = sr.expected_sums_pairs(fix, metric, fix["T"], fix["pairs0"])[1]
            Tn, R, t64 = sr.solve_step(metric, sums, fix["T"], fix["smt0"], fix["dst_mean"])
            off = float(np.abs(R - np.eye(3)).max())
            terr = float(np.abs(t64 - fix["T1"][:3, 3].astype(np.float64)).max())
            worst[(tname, metric)] = (off, terr)
            # the f32 half-ulp, by construction: the translation rounds to the predicted one, the linear part's noise is absorbed
            assert np.array_equal(Tn[:3, 3], fix["T1"][:3, 3]), (nd, tname, metric, terr)
            assert off < sr.ABSORB and np.abs(Tn[:3, :3] - fix["T"][:3, :3]).max() < sr.ABSORB
            assert np.array_equal(sr.transform_points(Tn, fix["S"], np.float32), fix["q1"]), (nd, tname, metric, off)
            assert np.array_equal(sr.transform_points(Tn, fix["src_mean"].reshape(1, 3), np.float32)[0], fix["smt1"])
        # ... and so is anything up to ABSORB in every entry
        for _ in range(4):
            Tp = fix["T1"].copy()
            Tp[:3, :3] = (Tp[:3, :3].astype(np.float64) + sr.ABSORB * rng.choice([-1.0, 1.0], (3, 3))).astype(np.float32)
            assert not np.array_equal(Tp, fix["T1"])
            assert np.array_equal(sr.transform_points(Tp, fix["S"], np.float32), fix["q1"])
            assert np.array_equal(sr.transform_points(Tp, fix["src_mean"].reshape(1, 3), np.float32)[0], fix["smt1"])
    print("first step", nd, "largest |R - I| entry, largest f64 translation error:", max(v[0] for v in worst.values()), max(v[1] for v in worst.values()))


@pytest.mark.parametrize("nd", SIZES)
def test_second_iteration_restatement_is_the_oracles(orc, nd):
    """orc.estimate_p2p's moments and orc.estimate_combined's AtA / Atb (MODE_MIXED) over the iteration-1 pair lists under T1"""
    for tname in TNAMES:
        fix = sr.two_step_pair(nd, tname)
        q = orc.transform_points(fix["T1"], fix["S"])
        assert np.array_equal(q, fix["q1"])
        smt = orc.transform_points(fix["T1"], fix["src_mean"].reshape(1, 3))[0]
        assert np.array_equal(smt, fix["smt1"])
        for d in ("first_to_second", "both_reciprocal"):
            ti, si = fix["pairs1"][d]
            _T, sums, _ok = orc.estimate_p2p(fix["D"], q, ti, si, orc.MODE_MIXED)
            assert np.array_equal(sums, sr.expected_sums_pairs(fix, sr.KABSCH, fix["T1"], (ti, si))[1][:16]), (nd, tname, d)
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                metric = sr.metric_of_weights(w_p2p, w_p2pl)
                assert (w_p2p, w_p2pl) == sr.METRIC_WEIGHTS[metric]
                _T, AtA, Atb, _cv = orc.estimate_combined(fix["D"], fix["N"], q, ti, si, w_p2p, w_p2pl, fix["dst_mean"], smt, 1, 1e-5, orc.MODE_MIXED)
                eA, eb = sr.gn_normal_equations(sr.expected_sums_pairs(fix, metric, fix["T1"], (ti, si))[1], w_p2p, w_p2pl)
                assert np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (nd, tname, d, w_p2p, w_p2pl)


def test_second_iteration_sums_notice_a_wrong_pair():
    """what a wrong k_reverse_warm amounts to changes the expected vector AND the transform after it: a pair of any group dropped (the last
    round's, a listed one's), a listed pair counted twice, a twin counted under mode 3 or left out under mode 2, the normal of another
    target point on a settled (residual-free) A pair"""
    for nd in (255, 2049):
        fix = sr.two_step_pair(nd, "rz90_shift")
        ti, si = fix["pairs1"]["first_to_second"]
        grp = np.concatenate([fix["group"][si[:len(si) - len(fix["tw_t"])]], np.full(len(fix["tw_t"]), 3)])
        for metric in sr.METRICS:
            base, f64 = sr.expected_sums_pairs(fix, metric, fix["T1"], (ti, si))
            T2 = sr.solve_step(metric, f64, fix["T1"], fix["smt1"], fix["dst_mean"])[0]
            for g in (sr.GROUP_A, sr.GROUP_B, 3):
                k = int(np.nonzero(grp == g)[0][0])
                keep = np.arange(len(ti)) != k
                dropped, d64 = sr.expected_sums_pairs(fix, metric, fix["T1"], (ti[keep], si[keep]))
                twice, t64 = sr.expected_sums_pairs(fix, metric, fix["T1"], (np.append(ti, ti[k]), np.append(si, si[k])))
                assert dropped != base and twice != base
                for other in (d64, t64):
                    assert not np.array_equal(sr.solve_step(metric, other, fix["T1"], fix["smt1"], fix["dst_mean"])[0], T2), (nd, metric, g)
            if metric in (sr.PLANE, sr.BOTH):
                k = int(np.nonzero(grp == sr.GROUP_A)[0][0])
                N2 = fix["N"].copy()
                N2[ti[k]] = fix["N"][ti[(k + 1) % len(ti)]]
                assert not np.array_equal(N2[ti[k]], fix["N"][ti[k]])
                stale = sr.expected_sums(metric, fix["D"], N2, fix["S"][si], fix["T1"], fix["dst_mean"], fix["src_mean"], ti, np.ones(len(ti), bool))
                assert stale[0] != base
                assert not np.array_equal(sr.solve_step(metric, stale[1], fix["T1"], fix["smt1"], fix["dst_mean"])[0], T2)


def test_reverse_walk_meets_a_sites_and_twins_at_its_edges():
    """in the order the reverse kernels walk the target (grid_order: the grid's cell-major sort, restated; the GPU test compares the shape
    with the library's): at some size an A site and a twin in the last round, in lane 0 and in lane 63 of a wave"""
    seen = {}
    for nd in DENSE:
        _g, places = sr.reverse_walk_places(sr.two_step_pair(nd))
        for name, cnt in places.items():
            for where, v in cnt.items():
                if where == "last_round" and nd % 256 == 0 and nd // 256 == 1:
                    continue      # (a single full round is the last one trivially; counted at the sizes with a partly filled one)
                seen[(name, where)] = seen.get((name, where), 0) + v
    for name in ("a", "twin"):
        for where in ("last_round", "lane0", "lane63"):
            assert seen[(name, where)] > 0, (name, where, seen)
    # the large target: 32,770 rounds over 2,048 blocks, so block 0 walks 17 and flushes once inside its loop, after 16 rounds; a wave whose
    # 16 x 64 points hold no A site (the only settled ones) has listed all of them by then: RW_WCAP entries exactly
    fix = sr.two_step_pair(sr.TWO_STEP_LARGE)
    g = sr.grid_order(fix["D"])
    assert g["occupancy"] <= 3.0
    pos = np.empty(fix["nd"], np.int64)
    pos[g["order"]] = np.arange(fix["nd"])
    pa = pos[fix["site_t"][fix["group"] == sr.GROUP_A]]
    rounds = (fix["nd"] + 255) // 256
    assert rounds == 16 * 2048 + 2 and len(range(0, rounds, 2048)) == 17
    first16 = pa[((pa // 256) % 2048 == 0) & ((pa // 256) // 2048 < 16)]
    settled_per_wave = np.bincount((first16 % 256) // 64, minlength=4)
    assert (settled_per_wave == 0).any(), settled_per_wave
    print("reverse walk", seen, "A sites in block 0's first 16 rounds, per wave:", settled_per_wave.tolist())
