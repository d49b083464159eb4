"""GPU: cilhip_knn_nd / cilhip_radius_search_nd and their mirrors against the yardstick of tests/_knn_nd_refs.py.
Indices, counts and offsets must be exact and every d2 must match bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _knn_nd_refs as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INF = float("inf")
F32 = np.float32


def _lib():
    from cilantro_amd import capi

    return capi.load()


def gpu_knn(ref, qry, k, bound=INF, want_d2=True, want_cnt=True):
    """the C entry on host arrays -> (idx int64 with -1, d2, cnt) as the yardstick returns them"""
    from cilantro_amd import capi

    ref = np.ascontiguousarray(ref, F32)
    nq = len(ref) if qry is None else len(qry)
    qry = None if qry is None else np.ascontiguousarray(qry, F32)
    idx = np.full((nq, k), 12345, np.uint32); d2 = np.full((nq, k), 7, F32); cnt = np.full(nq, 12345, np.uint32)
    rc = _lib().cilhip_knn_nd(0, ref.ctypes.data, len(ref), None if qry is None else qry.ctypes.data, nq, ref.shape[1], 0, k, C.c_float(bound), idx.ctypes.data,
                              d2.ctypes.data if want_d2 else None, cnt.ctypes.data if want_cnt else None)
    assert rc == capi.OK, _lib().cilhip_last_error(None).decode()
    out = idx.astype(np.int64)
    out[idx == capi.NONE_IDX] = -1
    return out, d2, cnt.astype(np.int64)


def gpu_radius(ref, qry, radius_sq):
    from cilantro_amd import kd_tree

    return kd_tree.KDTreeXf(np.ascontiguousarray(ref, F32)).radiusSearch(None if qry is None else np.ascontiguousarray(qry, F32), radius_sq)


def same_knn(got, want, what=""):
    assert np.array_equal(got[2], want[2]), ("counts", what)
    assert np.array_equal(got[0], want[0]), ("indices", what, int((got[0] != want[0]).sum()))
    assert np.array_equal(R.bits(got[1]), R.bits(want[1])), ("d2 bits", what, int((R.bits(got[1]) != R.bits(want[1])).sum()))


def same_radius(got, want, what=""):
    assert np.array_equal(got[0], want[0]), ("offsets", what)
    assert np.array_equal(got[1], want[1]), ("indices", what)
    assert np.array_equal(R.bits(got[2]), R.bits(want[2])), ("d2 bits", what)


def check_knn(ref, qry, k, bound=INF, what=""):
    got = gpu_knn(ref, qry, k, bound)
    same_knn(got, R.knn(ref, qry, k, bound), what)
    return got


# ---- every dimension -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", range(1, 17))
def test_every_dimension(dim):
    ref, qry = R.cloud(1500, dim, 20 + dim), R.cloud(300, dim, 60 + dim)
    got = check_knn(ref, qry, 10, what=dim)
    assert (got[2] == 10).all()
    # a radius near the 5th neighbour's distance: lists of about 5 entries, some empty, some long
    r2 = float(np.median(got[1][:, 4]))
    rad = gpu_radius(ref, qry, r2)
    same_radius(rad, R.radius(ref, qry, r2), dim)
    assert rad[0][-1] > len(qry)


# ---- the edges -----------------------------------------------------------------------------------------------------
N_REF_EDGES = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097, R.TILE - 1, R.TILE, R.TILE + 1})


@pytest.mark.parametrize("dim", [5, 6, 7, 9, 16])
def test_n_ref_edges(dim):
    pool, qry = R.cloud(4097, dim, 300 + dim), R.cloud(70, dim, 400 + dim)
    for n_ref in N_REF_EDGES:
        check_knn(pool[:n_ref], qry, 4, what=(dim, n_ref))
    r2 = float(dim) * 0.6
    for n_ref in (1, R.TILE - 1, R.TILE + 1, 257, 4097):
        same_radius(gpu_radius(pool[:n_ref], qry, r2), R.radius(pool[:n_ref], qry, r2), (dim, n_ref))


@pytest.mark.parametrize("n_query", [1, 255, 256, 257])
def test_n_query_edges(n_query):
    ref, qry = R.cloud(300, 6, 11), R.cloud(n_query, 6, 12)
    check_knn(ref, qry, 5, what=n_query)
    same_radius(gpu_radius(ref, qry, 3.0), R.radius(ref, qry, 3.0), n_query)


@pytest.mark.parametrize("dim", [5, 6, 7, 9, 16])
def test_k_edges(dim):
    ref, qry = R.cloud(257, dim, 500 + dim), R.cloud(257, dim, 600 + dim)
    for k in (1, 2, 31, 32):
        check_knn(ref, qry, k, what=(dim, k))
    got = check_knn(ref[:5], qry, 8, what="k > n_ref")
    assert (got[2] == 5).all() and (got[0][:, 5:] == -1).all() and np.isinf(got[1][:, 5:]).all()
    # the optional outputs are optional
    only = gpu_knn(ref, qry, 3, want_d2=False, want_cnt=False)
    assert np.array_equal(only[0], R.knn(ref, qry, 3)[0]) and (only[1] == 7).all() and (only[2] == 12345).all()


def test_self_search_finds_each_point_first():
    for dim in (2, 9):
        ref = R.cloud(700, dim, 31 + dim)
        got = check_knn(ref, None, 6, what=dim)
        assert np.array_equal(got[0][:, 0], np.arange(700)) and (got[1][:, 0] == 0).all()
        same_radius(gpu_radius(ref, None, 0.5), R.radius(ref, None, 0.5), dim)


def test_host_and_device_memory_agree():
    import torch
    from cilantro_amd import kd_tree

    ref, qry = R.cloud(1025, 7, 41), R.cloud(300, 7, 42)
    host = kd_tree.KDTreeXf(ref)
    dev = kd_tree.KDTreeXf(torch.from_numpy(ref).cuda())
    dq = torch.from_numpy(qry).cuda()
    want = R.knn(ref, qry, 10)
    for got in (host.kNNSearch(qry, 10), dev.kNNSearch(dq, 10)):
        same_knn(got, want)
    same_knn(dev.kNNSearch(None, 3), R.knn(ref, None, 3))
    a, b = host.radiusSearch(qry, 4.0), dev.radiusSearch(dq, 4.0)
    same_radius(a, R.radius(ref, qry, 4.0))
    same_radius(b, a)
    same_knn(dev.kNNInRadiusSearch(dq, 5, 4.0), R.knn(ref, qry, 5, 4.0))
    i, d = dev.nearestNeighborSearch(dq)
    assert np.array_equal(i, want[0][:, 0]) and np.array_equal(R.bits(d), R.bits(want[1][:, 0]))
    with pytest.raises(ValueError):
        dev.kNNSearch(qry, 2)      # one memory space per call


def test_the_bound_is_strict():
    ref, qry = R.cloud(600, 6, 51), R.cloud(40, 6, 52)
    k = 8
    plain = check_knn(ref, qry, k)
    kth = plain[1][0, k - 1]
    assert kth > plain[1][0, k - 2]
    below, above = np.nextafter(kth, F32(0)), np.nextafter(kth, F32(np.inf))
    for bound, want0 in ((below, k - 1), (kth, k - 1), (above, k)):
        got = check_knn(ref, qry, k, float(bound), what=float(bound))
        assert got[2][0] == want0


def test_exact_ties_go_to_the_lowest_index():
    base = R.cloud(200, 5, 61)
    doubled = np.concatenate([base, base[:80], base[:30]])      # rows 0..29 three times, 30..79 twice
    perm = np.random.default_rng(62).permutation(len(doubled))
    ref = doubled[perm]
    for k in (1, 2, 3, 7):
        check_knn(ref, R.cloud(100, 5, 63), k, what=k)
        got = check_knn(ref, None, k, what=("self", k))
        assert (got[1][:, 0] == 0).all()
    axis = np.arange(5, dtype=F32)
    lattice = np.stack(np.meshgrid(axis, axis, axis, axis, indexing="ij"), -1).reshape(-1, 4)[np.random.default_rng(64).permutation(625)]
    qry = np.concatenate([lattice[:60], lattice[:60] + F32(0.5)])
    for k in (1, 4, 9, 32):
        got = check_knn(lattice, qry, k, what=("lattice", k))
        assert k == 1 or (np.diff(got[1], axis=1) == 0).any()      # the lists do hold equal distances
    same_radius(gpu_radius(lattice, qry, 2.5), R.radius(lattice, qry, 2.5))
    same_radius(gpu_radius(ref, None, 1e-30), R.radius(ref, None, 1e-30))      # only the copies


def test_dim_3_equals_knn3f_under_tie_rule_0():
    from cilantro_amd import normal_estimation as ne

    ref, qry = R.cloud(3000, 3, 71), R.cloud(400, 3, 72)
    ref[100:140] = ref[:40]      # some exact ties
    ne.set_knn_tie_rule(0)
    try:
        for k, bound in ((10, np.inf), (32, np.inf), (6, 0.05)):
            want = ne.KDTree3f(ref).kNNSearch(qry, k) if bound == np.inf else ne.KDTree3f(ref).kNNInRadiusSearch(qry, k, bound)
            same_knn(gpu_knn(ref, qry, k, bound), want, (k, bound))
        want = ne.KDTree3f(ref).kNNSearch(None, 5)
        same_knn(gpu_knn(ref, None, 5), want, "self")
    finally:
        ne.set_knn_tie_rule(2)


def test_non_finite_points_and_overflow():
    for dim in (2, 6, 9):
        ref, qry = R.cloud(400, dim, 81 + dim), R.cloud(60, dim, 91 + dim)
        ref[3, 0] = np.nan; ref[4, dim - 1] = np.inf; ref[5, dim // 2] = -np.inf; ref[6] = np.nan
        ref[7, dim - 1] = 1e20; ref[8, 0] = -1e20      # finite, but d2 overflows
        qry[0, 0] = np.nan; qry[1, dim - 1] = np.inf; qry[2] = -np.inf; qry[3, 0] = 1e20
        for k, bound in ((10, INF), (3, 2.0)):
            got = check_knn(ref, qry, k, bound, what=(dim, k))
            assert got[2][:4].tolist() == [0, 0, 0, 0] and not np.isin(got[0], [3, 4, 5, 6, 7, 8]).any()
        got = check_knn(ref, None, 4)
        assert got[2][[3, 4, 5, 6]].tolist() == [0, 0, 0, 0] and got[0][7, 0] == 7 and got[2][7] == 1      # 1e20 finds itself and nothing else
        rad = gpu_radius(ref, qry, 3.0)
        same_radius(rad, R.radius(ref, qry, 3.0), dim)
        assert rad[0][4] == 0


# ---- radius search -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [5, 6, 7, 9, 16])
def test_radius_search(dim):
    from cilantro_amd import capi

    L = _lib()
    ref, qry = R.cloud(1025, dim, 700 + dim), R.cloud(257, dim, 800 + dim)
    pair = R.d2_matrix(ref, qry[:1])[0]
    d = np.sort(pair)[12]      # the 13th nearest point of query 0
    for r2, n0 in ((np.nextafter(d, F32(0)), 12), (d, 12), (np.nextafter(d, F32(np.inf)), 13)):
        got = gpu_radius(ref, qry, float(r2))
        same_radius(got, R.radius(ref, qry, float(r2)), (dim, float(r2)))
        assert got[0][1] == n0
    for r2 in (0.0, -0.0, -3.0):
        off, idx, d2 = gpu_radius(ref, qry, r2)
        assert (off == 0).all() and len(idx) == 0 and len(d2) == 0
    # the capacity protocol, on the entry itself
    r2 = float(d)
    want = R.radius(ref, qry, r2)
    total_want = int(want[0][-1])
    assert total_want > len(qry)
    for capacity in (0, total_want - 1, total_want):
        off = np.full(len(qry) + 1, 7, np.uint64); idx = np.full(total_want, 12345, np.uint32); d2 = np.full(total_want, 7, F32)
        total = C.c_size_t(0)
        rc = L.cilhip_radius_search_nd(0, ref.ctypes.data, len(ref), qry.ctypes.data, len(qry), dim, 0, C.c_float(r2), off.ctypes.data, idx.ctypes.data, d2.ctypes.data, capacity,
                                       C.byref(total))
        assert rc == capi.OK and total.value == total_want and np.array_equal(off.astype(np.int64), want[0])
        if capacity < total_want:
            assert (idx == 12345).all() and (d2 == 7).all()
        else:
            assert np.array_equal(idx.astype(np.int64), want[1]) and np.array_equal(R.bits(d2), R.bits(want[2]))
    # without distances, without a total
    off = np.zeros(len(qry) + 1, np.uint64); idx = np.zeros(total_want, np.uint32)
    assert L.cilhip_radius_search_nd(0, ref.ctypes.data, len(ref), qry.ctypes.data, len(qry), dim, 0, C.c_float(r2), off.ctypes.data, idx.ctypes.data, None, total_want, None) == capi.OK
    assert np.array_equal(idx.astype(np.int64), want[1])


def test_two_runs_are_bit_identical():
    ref, qry = R.cloud(4097, 9, 91), R.cloud(513, 9, 92)
    a, b = gpu_knn(ref, qry, 17), gpu_knn(ref, qry, 17)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    a, b = gpu_radius(ref, qry, 5.0), gpu_radius(ref, qry, 5.0)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)) and len(a[1]) > 0


# ---- end to end ----------------------------------------------------------------------------------------------------
def test_two_rings_end_to_end():
    import cilantro_amd
    from cilantro_amd import clustering as cl

    rng = np.random.default_rng(5)
    ang = 2 * np.pi * (np.arange(400) // 2) / 200 + rng.uniform(0, 0.01, 400)      # evenly spread, jittered
    planted = (np.arange(400) % 2).astype(np.int64)      # the rings interleaved
    rad = np.where(planted == 0, 1.0, 3.0) + rng.normal(0, 0.01, 400)
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1).astype(F32)
    tree = cilantro_amd.KDTree2f(pts)
    idx, d2, cnt = tree.kNNSearch(None, 10)
    same_knn((idx, d2, cnt), R.knn(pts, None, 10))
    assert (planted[idx] == planted[:, None]).all()      # every neighbour lies on the point's own ring
    W = cl.nn_graph_sparse_matrix((idx, d2), None, True)
    sc = cl.SpectralClustering(W, 2, False, initial_centroid_indices=[0, 1])
    W.close()
    assert sc.getNumberOfClusters() == 2 and (sc.getPointToClusterIndexMap() == planted).all()
    off, ridx, rd2 = tree.radiusSearch(None, 0.5 ** 2)
    same_radius((off, ridx, rd2), R.radius(pts, None, 0.25))
    labels, seg_off, members = cl.connected_components_from_lists(400, off, ridx)
    assert len(seg_off) == 3 and (labels[planted == 0] == labels[0]).all() and (labels[planted == 1] == labels[1]).all() and labels[0] != labels[1]


def test_example_prints_the_reference_examples_neighbours():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(ROOT, "examples", "kd_tree.cpp"), "example_kd_tree")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0].split() == ["Neighbor", "indices:", "0", "3"] and lines[1].split() == ["Neighbor", "distances:", "0.18", "0.38"], r.stdout
    assert lines[2] == "4-D:" and lines[3].split() == ["Neighbor", "indices:", "0", "4"] and lines[4].split() == ["Neighbor", "distances:", "0.22", "0.42"], r.stdout
