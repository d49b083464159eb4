"""Pins tests/_nonfinite_refs.py on the CPU: the expectations the GPU tests of clouds with NaN / +-inf points compare against (the
oracle on the filtered clouds, indices mapped back) equal a numpy brute force in f32 on the UNFILTERED arrays, where IEEE
comparisons alone keep a non-finite point out of every result; and every input those tests generate is free of ties.  This proves
the helpers, not the kernels."""
import numpy as np
import pytest

import _nonfinite_refs as nf

N = 500


@pytest.fixture(scope="module")
def case(orc):
    c = nf.pair_case(orc, N, "mixed", "mixed")
    c["r_list"] = np.float32((3.0 * c["h"]) ** 2)
    return c


def test_spoil_writes_each_kind():
    x = np.arange(30, dtype=np.float32).reshape(10, 3)
    y = nf.spoil(x, [0, 1, 2, 3, 4], nf.KINDS)
    assert np.isnan(y[0]).sum() == 1 and np.isnan(y[1]).all()
    assert (y[2] == np.inf).sum() == 1 and (y[3] == -np.inf).sum() == 1 and np.isfinite(y[2]).sum() == 2 and np.isfinite(y[3]).sum() == 2
    assert y[4, 0] == np.inf and y[4, 1] == -np.inf and y[4, 2] == x[4, 2]
    assert np.array_equal(y[5:], x[5:]) and np.array_equal(x, np.arange(30, dtype=np.float32).reshape(10, 3))      # a copy
    assert np.array_equal(nf.finite_mask(y), np.arange(10) >= 5)
    for name in nf.ROW_SETS:
        rows = nf.spoiled_rows(257, name)
        assert len(np.unique(rows)) == len(rows) and rows.min() >= 0 and rows.max() < 257
    assert len(nf.spoiled_rows(257, "run")) == 70 and np.all(np.diff(nf.spoiled_rows(257, "run")) == 1)
    assert list(nf.spoiled_rows(257, "first")) == [0] and list(nf.spoiled_rows(257, "last")) == [256]


def test_a_spoiled_source_row_is_a_spoiled_query(case, orc):
    """the pinned f32 transform spreads a non-finite coordinate over the row: filtering the queries is filtering the source rows"""
    assert np.array_equal(nf.finite_mask(case["q"]), nf.finite_mask(case["src"]))
    assert (~nf.finite_mask(case["src"])).sum() > 70 and (~nf.finite_mask(case["dst"])).sum() > 70


def test_expected_nn_is_the_brute_force_on_the_unfiltered_clouds(case, orc):
    di, si, dv, nn, nd2 = nf.expected_nn(orc, case["dst"], case["q"], case["max_sq"])
    lists = nf.brute_lists(case["dst"], case["q"], case["max_sq"], 1)
    want = np.array([l[0][0] if len(l[0]) else -1 for l in lists], np.int64)
    assert np.array_equal(nn, want) and 50 < (want >= 0).sum() < N
    assert np.array_equal(nd2[want >= 0].view(np.uint32), np.array([l[1][0] for l in lists if len(l[0])], np.float32).view(np.uint32))
    assert np.array_equal(si, np.nonzero(want >= 0)[0]) and np.array_equal(di, want[want >= 0]) and np.array_equal(dv, nd2[si])
    fd, fq = nf.finite_mask(case["dst"]), nf.finite_mask(case["q"])
    assert fd[di].all() and fq[si].all() and (nn[~fq] == -1).all()


@pytest.mark.parametrize("direction,reciprocal", [(1, False), (2, False), (2, True)])
def test_expected_dir_is_the_brute_force_on_the_unfiltered_clouds(case, orc, direction, reciprocal):
    di, si, dv = nf.expected_dir(orc, case["dst"], case["q"], case["max_sq"], direction, reciprocal)
    D = nf.brute_d2(case["dst"], case["q"])      # [nq, nd]
    with np.errstate(invalid="ignore"):
        ok = D < case["max_sq"]
    Dm = np.where(ok, D, np.float32(np.inf))
    fwd = {(int(Dm[j].argmin()), j) for j in range(len(D)) if ok[j].any()}            # every query's nearest target point
    rev = {(i, int(Dm[:, i].argmin())) for i in range(D.shape[1]) if ok[:, i].any()}  # every target point's nearest query
    want = sorted(rev if direction == 1 else ((fwd & rev) if reciprocal else (fwd | rev)))
    assert list(zip(di.tolist(), si.tolist())) == want and len(want) > 50
    assert np.array_equal(dv.view(np.uint32), np.array([D[j, i] for i, j in want], np.float32).view(np.uint32))


@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("self_query", [False, True])
def test_expected_knn_and_radius_are_the_brute_force_on_the_unfiltered_clouds(case, orc, k, self_query):
    ref = case["dst"]
    q = None if self_query else case["q"]
    qa = ref if self_query else q
    for r2 in (np.inf, case["r_list"]):
        idx, d2, cnt = nf.expected_knn(orc, ref, q, k, r2)
        lists = nf.brute_lists(ref, qa, r2, k)
        for i, (li, ld) in enumerate(lists):
            assert cnt[i] == len(li) and np.array_equal(idx[i, :len(li)], li) and (idx[i, len(li):] == -1).all(), (k, r2, i)
            assert np.array_equal(d2[i, :len(li)].view(np.uint32), ld.astype(np.float32).view(np.uint32)) and np.isinf(d2[i, len(li):]).all()
        assert (cnt[~nf.finite_mask(qa)] == 0).all() and np.isfinite(d2[idx >= 0]).all()
    if k == 1:
        for r2 in (0.0, case["r_list"]):
            off, idx, d2 = nf.expected_radius(orc, ref, q, r2)
            lists = nf.brute_lists(ref, qa, r2)
            assert np.array_equal(np.diff(off), [len(l[0]) for l in lists])
            assert np.array_equal(idx, np.concatenate([l[0] for l in lists]).astype(np.int64)) if len(idx) else sum(len(l[0]) for l in lists) == 0
            if len(idx):
                assert np.array_equal(d2.view(np.uint32), np.concatenate([l[1] for l in lists]).astype(np.float32).view(np.uint32))


def test_all_rows_spoiled_expect_nothing(orc):
    x = nf.spoil(np.zeros((5, 3), np.float32), np.arange(5), nf.KINDS)
    q = np.random.default_rng(1).random((7, 3), dtype=np.float32)
    assert len(nf.expected_nn(orc, x, q, 1.0)[0]) == 0 and len(nf.expected_nn(orc, q, x, 1.0)[0]) == 0
    assert len(nf.expected_dir(orc, x, q, 1.0, 2)[0]) == 0
    assert (nf.expected_knn(orc, x, q, 3)[2] == 0).all() and (nf.expected_knn(orc, x, None, 3)[2] == 0).all()
    assert nf.expected_radius(orc, x, q, 1.0)[0][-1] == 0


def test_the_small_inputs_are_tie_free_by_brute_force(case):
    assert nf.tie_free(case["dst"], case["q"], np.inf, 32) and nf.tie_free(case["dst"], case["dst"], np.inf, 32)


@pytest.mark.parametrize("n", nf.PAIR_SIZES)
def test_the_gpu_tests_inputs_are_tie_free(orc, n):
    """every input of tests/test_gpu_nonfinite.py: each query's nearest distance and the members of its 32-lists are unique (k + 1 = 33 nearest
    distances pairwise different), for the transformed source and for the target's own points as queries; the radius lists are sub-lists of these"""
    cases = [nf.pair_case(orc, n, a, b) for a, b in ((w, None) for w in nf.ROW_SETS)] if n == nf.PAIR_SIZES[0] else []
    cases += [nf.pair_case(orc, n, None, "mixed"), nf.pair_case(orc, n, "mixed", "mixed"), nf.pair_case(orc, n)]
    # (the finite-but-hostile case is not in the list: it holds no non-finite point, so its tie order IS defined -- the reference's -- and
    #  its far queries do see the whole cloud at equal f32 distances)
    for c in cases:
        assert nf.tie_free_oracle(orc, c["dst"], c["q"], np.inf, 32)
        assert nf.tie_free_oracle(orc, c["dst"], None, np.inf, 32)
        assert nf.tie_free_oracle(orc, c["q"], c["dst"], np.inf, 1)      # the reverse searches: every target point's nearest query


def test_the_hostile_case_outliers_have_in_range_matches(orc):
    c = nf.hostile_case(orc)
    D = nf.brute_d2(c["dst"][-2:], c["q"][-2:])
    assert D[0, 0] < c["max_sq"] and D[1, 1] < c["max_sq"] and D[0, 0] > 0 and D[1, 1] > 0
    assert np.isfinite(c["dst"]).all() and np.isfinite(c["src"]).all() and len(c["dst"]) == 20002 == len(c["src"])
