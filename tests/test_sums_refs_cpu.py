"""tests/_sums_refs.py held to its own conditions and to the CPU oracle, without a GPU: the fixtures of every case tests/test_gpu_exact_sums.py
runs are exact (f32 == f64 evaluation of every term, every sum inside 53 bits, used slots non-zero and apart, nearest neighbours unique), the
integer restatement of the 48 sums gives the oracle's own moments and normal equations bit for bit on the same lattices, and it notices
every mutation a wrong kernel could amount to."""
import numpy as np
import pytest

import _sums_refs as sr

ORACLE_SIZES = (1, 2, 65, 257, 2049, 65537)


@pytest.mark.parametrize("n", sr.SIZES)
def test_every_case_of_the_table_is_exact(n):
    """every size x transform x mask x metric of section A and C, the single-match fixtures, the symmetric kind and the weighted cases of B"""
    cases = 0
    for tname in sr.A_TRANSFORMS + (("mirror_z",) if n in sr.STORED_SIZES else ()):
        fix = sr.fixture(n, tname)
        assert fix["S"].dtype == np.float32 and fix["D"].dtype == np.float32
        for name, (r2, has) in sr.masks(fix).items():
            assert np.array_equal(has, fix["d2"] < r2) and not np.any(fix["d2"] == r2)
            for metric in sr.METRICS:
                sr.assert_exact_fixture(fix, metric, has, brute=(n <= 257 and tname == "identity" and name == "all"))
                cases += 1
        assert {"all", "none"} <= set(sr.masks(fix)) and (n < 3 or {"half", "all_but_one", "one"} <= set(sr.masks(fix)))
    if n in sr.SINGLE_SIZES:
        fix = sr.fixture(n)
        for k in range(n):
            g = sr.single_match_fixture(n, k)             # (the same query / transform pairing as the GPU test walks)
            assert g["tname"] == sr.A_TRANSFORMS[k % 2]
            r2, has = sr.masks(g)["one"]
            assert has.sum() == 1 and has[k] and np.array_equal(g["D"], fix["D"]) and np.array_equal(g["N"], fix["N"])
            for metric in sr.METRICS:
                sr.assert_exact_fixture(g, metric, has)
                cases += 1
    if n in sr.STORED_SIZES:
        for kind, tname in (("symmetric", "identity"), ("symmetric", "rz90_shift")):
            fix = sr.fixture(n, tname, kind)
            has = sr.masks(fix).get("half", sr.masks(fix)["all"])[1]
            for metric in (sr.PLANE, sr.BOTH):
                sr.assert_exact_fixture(fix, metric, has)
                cases += 1
        fix = sr.fixture(n)
        has = sr.masks(fix).get("half", sr.masks(fix)["all"])[1]
        wq, wp = sr.pair_weights(fix, has)
        for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
            sr.assert_exact_fixture(fix, sr.metric_of_weights(w_p2p, w_p2pl), has, weights=(np.float32(w_p2p) * wq, np.float32(w_p2pl) * wp))
            cases += 1
    assert cases >= 8


def test_slot_layout_on_one_hand_made_pair():
    """one pair, numbers small enough to follow by hand: the layout of solve.hpp:20-29"""
    D = np.array([[2, 5, 9]], np.float32); N = np.array([[0.5, -1.5, 2.0]], np.float32)
    S = np.array([[2.0625, 4.9375, 9.125]], np.float32)
    dm = np.array([1.0, 4.0, 8.0], np.float32); sm = np.array([1.5, 4.25, 8.5], np.float32)
    T = np.eye(4, dtype=np.float32)
    has = np.array([True])
    _n, k = sr.expected_sums(sr.KABSCH, D, N, S, T, dm, sm, [0], has)
    assert k[0] == 1 and list(k[1:4]) == [2, 5, 9] and list(k[4:7]) == [2.0625, 4.9375, 9.125] and k[7] == 2 * 2.0625 and k[9] == 2 * 9.125 and k[13] == 9 * 2.0625
    d = np.array([1.0, 1.0, 1.0]); s = np.array([0.5625, 0.6875, 0.625]); a = d + s; r = d - s; n = N[0].astype(np.float64)
    e = np.concatenate([np.cross(a, n), n]); res = float(n @ r)
    _n, p = sr.expected_sums(sr.BOTH, D, N, S, T, dm, sm, [0], has)
    tri = [e[i] * e[j] for i in range(6) for j in range(i, 6)]
    assert p[0] == 1 and list(p[1:22]) == tri and list(p[22:28]) == list(res * e)
    assert list(p[28:31]) == list(a) and list(p[31:37]) == [a[i] * a[j] for i in range(3) for j in range(i, 3)]
    assert list(p[37:40]) == list(np.cross(a, r)) and list(p[40:43]) == list(r) and p[43] == 1 and not p[44:].any()
    _n, q = sr.expected_sums(sr.POINT, D, N, S, T, dm, sm, [0], has)
    assert q[0] == 1 and not q[1:28].any() and np.array_equal(q[28:], p[28:])
    _n, l = sr.expected_sums(sr.PLANE, D, N, S, T, dm, sm, [0], has)
    assert np.array_equal(l[:28], p[:28]) and not l[28:].any()
    # per-pair weights: the plane block scales with wp, the point block with wq, slot 43 is the sum of wq, the count stays a count
    _n, w = sr.expected_sums(sr.BOTH, D, N, S, T, dm, sm, [0], has, weights=(np.array([0.5]), np.array([2.0])))
    assert w[0] == 1 and np.array_equal(w[1:28], 2.0 * p[1:28]) and np.array_equal(w[28:43], 0.5 * p[28:43]) and w[43] == 0.5


@pytest.mark.parametrize("n", ORACLE_SIZES)
def test_restatement_is_the_oracles_on_the_same_lattices(orc, n):
    """orc.estimate_p2p's 16 moments and orc.estimate_combined's AtA / Atb (MODE_MIXED: f32 terms, f64 sums -- the engine's contract) for
    the three dyadic weightings == gn_normal_equations over the exact sums, np.array_equal; symmetric objective and mirrored transform too"""
    for tname, kind in (("identity", "plain"), ("rz90_shift", "plain"), ("mirror_z", "plain"), ("rz90_shift", "symmetric")):
        fix = sr.fixture(n, tname, kind)
        q = orc.transform_points(fix["T"], fix["S"])
        assert np.array_equal(q, fix["q"])
        smt = orc.transform_points(fix["T"], fix["src_mean"].reshape(1, 3))[0]
        assert np.array_equal(smt, fix["smt"])
        snq = orc.transform_normals(fix["T"], fix["SN"]) if kind == "symmetric" else None
        if snq is not None:
            assert np.array_equal(snq, fix["SNq"])
        for name, (r2, has) in sr.masks(fix).items():
            si = np.nonzero(has)[0]
            di = fix["match"][si]
            if kind == "plain":
                _T, sums, _ok = orc.estimate_p2p(fix["D"], q, di, si, orc.MODE_MIXED)
                assert np.array_equal(sums, sr.expected_sums_of(fix, sr.KABSCH, has)[1][:16]), (n, tname, name)
            if len(si) == 0:
                continue
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                metric = sr.metric_of_weights(w_p2p, w_p2pl)
                _T, AtA, Atb, _cv = orc.estimate_combined(fix["D"], fix["N"], q, di, si, w_p2p, w_p2pl, fix["dst_mean"], smt, 1, 1e-5, orc.MODE_MIXED,
                                                          src_n_trans=snq)
                eA, eb = sr.gn_normal_equations(sr.expected_sums_of(fix, metric, has)[1], w_p2p, w_p2pl)
                assert np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, kind, name, w_p2p, w_p2pl)


@pytest.mark.parametrize("n", (1, 65, 257, 2049))
def test_affine_restatement_is_the_oracles(orc, n):
    """expected_affine == orc.estimate_affine's AtA[144] / Atb[12] (MODE_MIXED), centred (the dyadic means) and not (zero means).  Up to 2049
    points only: the oracle rounds every product of two f32 factors to f32 before it adds it up in f64 (oracle/estimator_impl.inc:
    (w * e[r]) * e[r2] in TERM), the engine forms the product in f64 (affine_device.hpp) -- the same number while it fits 24 bits, which
    the uncentred coordinates of the larger lattices (above 2^6, at 2^-4) no longer allow.  Beyond, expected_affine stands on the
    definition of solve.hpp:515-519 alone."""
    for tname in ("identity", "mirror_z"):
        fix = sr.fixture(n, tname)
        m = sr.masks(fix)
        has = m["half" if "half" in m else "all"][1]
        si = np.nonzero(has)[0]
        di = fix["match"][si]
        zero = np.zeros(3, np.float32)
        for centered in (False, True):
            sr.assert_exact_affine(fix, centered)
            dm, smt = (fix["dst_mean"], fix["smt"]) if centered else (zero, zero)
            for w_p2p, w_p2pl in sr.DYADIC_WEIGHTINGS:
                _T, AtA, Atb, _ok = orc.estimate_affine(fix["D"], fix["N"], fix["q"], di, si, w_p2p, w_p2pl, dm, smt, orc.MODE_MIXED)
                eA, eb, cnt = sr.expected_affine(fix, has, w_p2p, w_p2pl, centered)
                assert cnt == len(si) and np.array_equal(AtA, eA) and np.array_equal(Atb, eb), (n, tname, centered, w_p2p, w_p2pl)


def test_affine_terms_exact_at_the_stored_sizes():
    for n in sr.STORED_SIZES:
        for centered in (False, True):
            sr.assert_exact_affine(sr.fixture(n), centered)


def test_f64_matrix_product_is_the_integer_one():
    """above 4096 pairs the restatement forms z^T W z by an f64 matrix product: the same integers as the int64 product"""
    fix = sr.fixture(65537)
    has = sr.masks(fix)["half"][1]
    idx = np.nonzero(has)[0]
    q = sr.transform_points(fix["T"], fix["S"][idx], np.float64)
    mi = fix["match"][idx]
    z = sr.pair_terms(sr.BOTH, fix["D"][mi], fix["N"][mi], q, fix["dst_mean"], fix["smt"], np.float64)
    zi = np.rint(z * sr.ZSCALE).astype(np.int64)
    w = np.random.default_rng(0).integers(0, 17, len(idx)).astype(np.int64)
    assert sr._gram(zi, w) == sr._gram(zi, w, force_int=True)


def test_oracle_neighbours_are_the_fixtures(orc):
    """the lattice construction against a search: the oracle's exhaustive nearest neighbour under every mask's radius"""
    for n in (1, 2, 65, 257, 2049):
        fix = sr.fixture(n, "rz90_shift")
        for name, (r2, has) in sr.masks(fix).items():
            bi, bd = orc.nn_brute(fix["D"], fix["q"], float(r2))
            assert np.array_equal(bi >= 0, has) and np.array_equal(bi[has], fix["match"][has]), (n, name)
            assert np.array_equal(np.asarray(bd, np.float32)[has], fix["d2"][has])
            assert orc.count_ties_brute(fix["D"], fix["q"], float(r2)) == 0


def test_reference_notices_every_mutation():
    """what a wrong kernel amounts to must change the expected vector: any single pair dropped, the last pair counted twice, two slots
    swapped, n_z zeroed"""
    for n in (2, 65, 257):
        fix = sr.fixture(n, "rz90_shift")
        has = sr.masks(fix)["all"][1]
        for metric in sr.METRICS:
            base, _ = sr.expected_sums_of(fix, metric, has)
            used = [s for s in sr.used_slots(metric) if s != 43]
            for k in range(n):                            # dropping any single pair
                h = has.copy(); h[k] = False
                assert sr.expected_sums_of(fix, metric, h)[0] != base, (n, metric, k)
            # the last pair twice: the same fixture with that pair appended
            dup = np.concatenate([np.arange(n), [n - 1]])
            twice, _ = sr.expected_sums(metric, fix["D"], fix["N"], fix["S"][dup], fix["T"], fix["dst_mean"], fix["src_mean"], fix["match"][dup], np.ones(n + 1, bool))
            assert twice != base and twice[0] == base[0] + (1 << sr.DEN_LOG2)
            for i in range(len(used)):                    # swapping two used slots
                for j in range(i + 1, len(used)):
                    sw = list(base); sw[used[i]], sw[used[j]] = sw[used[j]], sw[used[i]]
                    assert sw != base, (n, metric, used[i], used[j])
            if metric in (sr.PLANE, sr.BOTH):             # the plane vector without n_z (rank_update.hpp: head comment)
                N0 = fix["N"].copy(); N0[:, 2] = 0.0
                assert sr.expected_sums(metric, fix["D"], N0, fix["S"], fix["T"], fix["dst_mean"], fix["src_mean"], fix["match"], has)[0] != base


def test_radius_between_and_masks():
    v = np.array([3, 10, 10, 14, 27], np.float32) / np.float32(256)
    assert [int((v < sr.radius_between(v, k)).sum()) for k in range(5)] == [0, 1, 3, 4, 5]
    with pytest.raises(AssertionError):
        sr.radius_between(v, 5)
    fix = sr.fixture(257)
    m = sr.masks(fix)
    assert [int(m[k][1].sum()) for k in ("all", "none", "all_but_one", "one")] == [257, 0, 256, 1] and 64 < m["half"][1].sum() < 192
    assert not m["all_but_one"][1][fix["far"]] and m["one"][1][fix["lone"]]
