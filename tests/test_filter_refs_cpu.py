"""Pins tests/_filter_refs.py on the CPU: what tests/test_gpu_post_filters.py compares the post-filters and pair lists against.
Every small fixture is on the exact lattice, free of nearest-neighbour ties in the search it is used for (brute force over the
pinned f32 d2), and its correspondence sets BY CONSTRUCTION are the brute force's; every function of the restatement equals the
oracle's (orc_filter_fraction, orc_filter_fraction_lex, orc_filter_one_to_one, orc_filter_one_to_one_f2s, find_correspondences_dir)
on every small fixture and every fraction.  This proves the helpers, not the kernels."""
import numpy as np
import pytest

import _filter_refs as fr

SIDE = 8


def _small_fixtures():
    full = fr.attached(SIDE, 1)
    out = [full, fr.attached(SIDE, 2, planar=True), fr.attached(SIDE, 3, tied=True), fr.shared(SIDE, 4), fr.shared(SIDE, 5, midpoint=True)]
    out += [fr.cut_matches(full, m) for m in fr.COUNTS]
    out.append(fr.cut_sources(fr.attached(12, 6), 4099))
    return out


@pytest.fixture(scope="module")
def fixtures():
    return _small_fixtures()


def _fractions(n):
    return list(fr.FRACTIONS) + fr.half_fractions(n)


def _call3(fn, t, *args):
    a = np.ascontiguousarray(t[0], np.int64).copy(); b = np.ascontiguousarray(t[1], np.int64).copy(); v = np.ascontiguousarray(t[2], np.float32).copy()
    n = fn(a, b, v, len(a), *args)
    return a[:n], b[:n], v[:n]


def test_fixtures_are_exact_and_free_of_nearest_neighbour_ties(orc, fixtures):
    report = {}
    for fix in fixtures:
        for x in (fix["dst"], fix["q"]):
            u = x.astype(np.float64) * 1024.0
            assert np.array_equal(u, np.round(u)) and np.abs(x).max() < 64.0, fix["name"]
        assert len(np.unique(fix["dst"], axis=0)) == len(fix["dst"])
        for side, pts, queries in (("fwd", fix["dst"], fix["q"]), ("rev", fix["q"], fix["dst"])):
            t = fix[side]
            if t is None:      # (this search ties by design: the fixture is not used in that direction)
                assert orc.count_ties_brute(pts, queries, fix["max_sq"]) > 0, (fix["name"], side)
                continue
            assert orc.count_ties_brute(pts, queries, fix["max_sq"]) == 0, (fix["name"], side)
            bi, bd = orc.nn_brute(pts, queries, fix["max_sq"])
            found = np.nonzero(bi >= 0)[0]
            got = (bi[found], found, bd[found]) if side == "fwd" else (found, bi[found], bd[found])
            assert fr.same(t, got), (fix["name"], side)
        report[fix["name"]] = {"targets": len(fix["dst"]), "sources": len(fix["q"]), "fwd": None if fix["fwd"] is None else len(fix["fwd"][0]),
                               "rev": None if fix["rev"] is None else len(fix["rev"][0])}
    print(report)
    full = fixtures[0]
    # the strict radius is exercised, values repeat, and index order is not grid order
    assert full["on_radius"] > 0 and len(np.unique(fr.bits(full["fwd"][2]))) <= 24 < len(full["fwd"][0])
    assert not np.array_equal(np.lexsort(full["dst"].T[::-1]), np.arange(len(full["dst"])))
    assert [len(f["fwd"][0]) for f in fixtures[5:5 + len(fr.COUNTS)]] == list(fr.COUNTS)
    assert len(fixtures[-1]["q"]) == 4099


def test_tie_fixtures_hold_the_ties_they_are_for(fixtures):
    tied, sh, mid = fixtures[2], fixtures[3], fixtures[4]
    assert fr.contended(tied["fwd"], 0)[1] > 20            # targets whose smallest value two or more sources hold
    c, m = fr.contended(sh["rev"], 1)
    assert c == sh["shared_sources"] > 20 and m == 0       # sources two targets name, at 60 and 68 units
    c, m = fr.contended(mid["rev"], 1)
    assert c == m == mid["shared_sources"] > 20            # ... at 64 and 64
    assert fr.contended(fixtures[0]["fwd"], 0)[1] == 0     # `attached`: the smallest value of a target is never shared


def test_keep_count_is_llround(orc):
    """against the C library's llround, through orc_filter_fraction's returned count"""
    halves = 0
    for n in list(range(0, 70)) + [255, 256, 257, 901, 65537]:
        t = (np.zeros(n, np.int64), np.arange(n, dtype=np.int64), np.zeros(n, np.float32))
        for f in _fractions(n) + [0.25, 0.75, 1.0 / 3.0, 0.1]:
            if 0.0 < f < 1.0:
                assert fr.keep_count(f, n) == len(orc.filter_fraction(*t, f)[0]), (n, f)
                halves += (f * n) % 1.0 == 0.5
    assert halves > 100
    assert fr.keep_count(0.25, 2) == 1 and fr.keep_count(0.5, 1) == 1 and fr.keep_count(0.5, 5) == 3      # round() gives 0, 0, 2
    for n in (2, 3, 6, 63, 64, 65, 255, 256, 257):
        hf = fr.half_fractions(n)
        assert hf and all((f * n) % 1.0 == 0.5 for f in hf), n


def test_each_filter_equals_the_oracles(orc, fixtures):
    L = orc.lib()
    for fix in fixtures:
        lists = []
        if fix["fwd"] is not None:
            lists.append(fix["fwd"])
        if fix["rev"] is not None:
            lists.append(fix["rev"])
        if fix["fwd"] is not None and fix["rev"] is not None:
            lists += [fr.union(fix["rev"], fix["fwd"]), fr.intersection(fix["rev"], fix["fwd"])]
        for t in lists:
            assert fr.same(fr.one_to_one_s2f(t), orc.filter_one_to_one(*t)), fix["name"]
            assert fr.same(fr.one_to_one_f2s(t), _call3(L.orc_filter_one_to_one_f2s, t)), fix["name"]
            for f in _fractions(len(t[0])):
                assert fr.same(fr.fraction_s2f(t, f), orc.filter_fraction(*t, f)), (fix["name"], f)
                assert fr.same(fr.fraction_pairs(t, f), _call3(L.orc_filter_fraction_lex, t, float(f))), (fix["name"], f)


def test_expected_lists_equal_the_oracles_end_to_end(orc, fixtures):
    for fix in fixtures:
        dirs = []
        if fix["fwd"] is not None:
            dirs.append((fr.S2F, False))
        if fix["rev"] is not None:
            dirs.append((fr.F2S, False))
        if fix["fwd"] is not None and fix["rev"] is not None:
            dirs += [(fr.BOTH, False), (fr.BOTH, True)]
        for d, recip in dirs:
            n = len(fr.expected(fix, d, recip)[0])
            for f in _fractions(n):
                for o2o in (False, True):
                    exp = fr.expected(fix, d, recip, f, o2o)
                    ref = orc.find_correspondences_dir(fix["dst"], fix["q"], fix["max_sq"], d, recip, f, o2o)
                    assert fr.same(exp, ref), (fix["name"], d, recip, f, o2o, len(exp[0]), len(ref[0]))


def test_stored_sources_transform_back_bit_for_bit(orc, fixtures):
    for name, (T, _) in fr.TRANSFORMS.items():
        fix = fixtures[1] if name == "flatten_z" else fixtures[0]
        s = fr.stored_source(fix["q"], name)
        assert np.array_equal(orc.transform_points(T, s), fix["q"]), name
        assert name == "identity" or not np.array_equal(s, fix["q"])
