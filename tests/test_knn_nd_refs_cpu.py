"""CPU: the yardstick of DESIGN.md section 21 (tests/_knn_nd_refs.py) and everything of the N-D neighbour search that needs no device.
  * rule N1 as the yardstick states it is the reference's nanoflann: 1-NN in 6 and 9 dimensions, k-NN lists in 3, index and distance bits
  * its neighbour sets agree with an f64 argsort wherever the f64 gap at the k-th place exceeds dim * 2^-21 * d2
  * the argument rules N4 of both entries without a device, outputs untouched; the calls that need no device
  * csrc/knn_nd_host.hpp stand-alone (tests/cpp/test_knn_nd_host.cpp), built plainly and under ASan / UBSan
  * the C++ mirror and the example compile
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _knn_nd_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INF = float("inf")


def _no_ties(d2):
    """no query's two smallest distances are equal"""
    two = np.sort(d2, axis=1)[:, :2]
    return bool((two[:, 0] != two[:, 1]).all())


# ---- the yardstick against the reference's own search --------------------------------------------------------------
@pytest.mark.parametrize("dim", [6, 9])
@pytest.mark.parametrize("seed", [1, 2])
def test_1nn_equals_the_reference_nanoflann(orc, dim, seed):
    ref, qry = R.cloud(3000, dim, seed), R.cloud(700, dim, 100 + seed)
    assert _no_ties(R.d2_matrix(ref, qry))
    idx, d2, cnt = R.knn(ref, qry, 1)
    find = orc.find_correspondences_feat6 if dim == 6 else orc.find_correspondences_feat9
    di, si, dv = find(ref, qry, 1e30, use_ref=orc.ref_available())
    assert si.tolist() == list(range(len(qry))) and (cnt == 1).all()
    mism = int((di != idx[:, 0]).sum()) + int((R.bits(dv) != R.bits(d2[:, 0])).sum())
    print("dim", dim, "seed", seed, "mismatches", mism, "reference's own nanoflann" if orc.ref_available() else "oracle restatement")
    assert mism == 0


def test_knn_lists_in_3d_equal_the_reference(orc):
    ref, qry = R.cloud(3000, 3, 7), R.cloud(500, 3, 8)
    k = 10
    full = np.sort(R.d2_matrix(ref, qry), axis=1)[:, :k + 1]
    assert (np.diff(full, axis=1) != 0).all()      # no equal distances among a query's k + 1 smallest: the lists are the same under any tie order
    idx, d2, cnt = R.knn(ref, qry, k)
    tree = orc.KDTree(ref, use_ref=orc.ref_available())
    if orc.ref_available():
        ri, rd, rc = orc.ref_knn_batch(tree, qry, k)
    else:
        rows = [tree.knn_in_radius(q, k, np.finfo(np.float32).max) for q in qry]
        ri, rd, rc = np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.full(len(qry), k)
    assert (np.asarray(rc) == k).all() and (cnt == k).all()
    assert np.array_equal(ri, idx) and np.array_equal(R.bits(rd), R.bits(d2))


@pytest.mark.parametrize("dim", range(1, 17))
def test_neighbour_sets_agree_with_f64(dim):
    """the f32 d2 of N1 carries at most (dim + 2) roundings of relative size 2^-24 each on non-negative terms; two of them differ from their exact
    values by less than 2 (dim + 2) 2^-24 d2 <= dim 2^-21 d2: beyond that gap the k nearest are the exact ones"""
    k = 10
    ref, qry = R.cloud(1500, dim, 20 + dim), R.cloud(300, dim, 60 + dim)
    idx, _, cnt = R.knn(ref, qry, k)
    exact = ((qry.astype(np.float64)[:, None, :] - ref.astype(np.float64)[None, :, :]) ** 2).sum(axis=2)
    order = np.argsort(exact, axis=1, kind="stable")
    ds = np.take_along_axis(exact, order, axis=1)
    clear = (ds[:, k] - ds[:, k - 1]) > dim * 2.0 ** -21 * ds[:, k]
    print("dim", dim, "queries with a clear k-th place:", int(clear.sum()), "of", len(qry))
    assert clear.sum() >= (len(qry) // 2 if dim > 1 else 1)
    assert (cnt == k).all()
    for i in np.nonzero(clear)[0]:
        assert set(idx[i].tolist()) == set(order[i, :k].tolist()), (dim, i)


def test_the_tail_is_added_one_coordinate_at_a_time():
    """dim = 6 is (g0 + s4) + s5, not g0 + (s4 + s5): values chosen so that the two differ"""
    q = np.zeros((1, 6), np.float32)
    p = np.zeros((1, 6), np.float32)
    p[0, 0] = 4096.0                        # g0 = 2^24
    p[0, 4] = p[0, 5] = 1.0                 # s4 = s5 = 1: (2^24 + 1) + 1 = 2^24 (ties to even twice), 2^24 + (1 + 1) = 2^24 + 2
    assert R.d2_matrix(p, q)[0, 0] == np.float32(2.0 ** 24)
    # and dim = 3 is ((s0 + s1) + s2)
    a, b = R.cloud(50, 3, 3), R.cloud(40, 3, 4)
    t = b[:, None, :] - a[None, :, :]
    assert np.array_equal(R.bits(R.d2_matrix(a, b)), R.bits((t[..., 0] * t[..., 0] + t[..., 1] * t[..., 1]) + t[..., 2] * t[..., 2]))


def test_yardstick_rules_n2_n3_n5():
    ref = np.array([[0, 0], [1, 0], [1, 0], [np.nan, 0], [np.inf, 1], [1e20, 0], [0, 1]], np.float32)
    qry = np.array([[0, 0], [np.nan, 0], [np.inf, 0]], np.float32)
    idx, d2, cnt = R.knn(ref, qry, 4)
    assert idx[0].tolist() == [0, 1, 2, 6] and d2[0].tolist() == [0, 1, 1, 1] and cnt.tolist() == [4, 0, 0]      # ties by index; 1e20 overflows: in no list
    idx, d2, cnt = R.knn(ref, qry, 8)
    assert idx[0].tolist() == [0, 1, 2, 6, -1, -1, -1, -1] and np.isinf(d2[0, 4:]).all() and cnt[0] == 4
    assert R.knn(ref, qry, 4, 1.0)[2].tolist() == [1, 0, 0]      # strict
    off, ii, dd = R.radius(ref, qry, np.nextafter(np.float32(1), np.float32(2)))
    assert off.tolist() == [0, 4, 4, 4] and ii.tolist() == [0, 1, 2, 6]
    assert R.radius(ref, qry, 0.0)[0].tolist() == [0, 0, 0, 0] and R.radius(ref, None, 1.0)[0].tolist() == [0, 1, 3, 5, 5, 5, 6, 7]


# ---- argument rules, without a device ------------------------------------------------------------------------------
def _err(L):
    return L.cilhip_last_error(None).decode()


def test_symbols_are_listed():
    from cilantro_amd import build, capi

    assert "cilhip_knn_nd" in capi.SYMBOLS and "cilhip_radius_search_nd" in capi.SYMBOLS
    assert "knn_nd.hip" in build.SOURCES and "knn_lists.hpp" in build.HEADERS and "knn_nd_host.hpp" in build.HEADERS
    host = open(os.path.join(ROOT, "cilantro_amd", "csrc", "knn_nd_host.hpp")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host      # plain C++
    # one copy of the list and of the radius tail
    knn, nd = (open(os.path.join(ROOT, "cilantro_amd", "csrc", f)).read() for f in ("knn.hip", "knn_nd.hip"))
    for needle in ("struct KList", "void k_unpack_radius", "segmented_radix_sort_keys"):
        assert needle not in knn and needle not in nd, needle
    m = re.search(r"constexpr int KNN_ND_TILE = (\d+);", nd)
    assert m and int(m.group(1)) == R.TILE and R.TILE <= 4096 and R.TILE & (R.TILE - 1) == 0


def test_knn_nd_refusals(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    ref = np.ones((8, 4), np.float32)
    idx = np.full((8, 3), 7, np.uint32); d2 = np.full((8, 3), 7, np.float32); cnt = np.full(8, 7, np.uint32)

    def call(r=ref.ctypes.data, n=8, q=None, nq=0, dim=4, mem=0, k=3, bound=INF, i=idx.ctypes.data):
        return L.cilhip_knn_nd(0, r, n, q, nq, dim, mem, k, C.c_float(bound), i, d2.ctypes.data, cnt.ctypes.data)

    for kwargs, code, needle in ((dict(r=None), capi.ERR_INVALID, "ref is NULL"), (dict(i=None), capi.ERR_INVALID, "idx_out is NULL"), (dict(dim=0), capi.ERR_INVALID, "dim is 0"),
                                 (dict(k=0), capi.ERR_INVALID, "k is 0"), (dict(bound=float("nan")), capi.ERR_INVALID, "max_sq_dist is NaN"),
                                 (dict(mem=2), capi.ERR_INVALID, "mem"), (dict(mem=-1), capi.ERR_INVALID, "mem"), (dict(n=2 ** 32 - 16), capi.ERR_INVALID, "2^32 - 16"),
                                 (dict(q=ref.ctypes.data, nq=2 ** 32 - 16), capi.ERR_INVALID, "2^32 - 16"), (dict(dim=17), capi.ERR_UNSUPPORTED, "dim > 16"),
                                 (dict(k=33), capi.ERR_UNSUPPORTED, "k > 32")):
        assert call(**kwargs) == code, kwargs
        assert needle in _err(L) and _err(L).startswith("knn_nd: "), (kwargs, _err(L))
        assert (idx == 7).all() and (d2 == 7).all() and (cnt == 7).all()


def test_radius_search_nd_refusals(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    ref = np.ones((8, 4), np.float32)
    off = np.full(9, 7, np.uint64); idx = np.full(64, 7, np.uint32); d2 = np.full(64, 7, np.float32)
    total = C.c_size_t(77)

    def call(r=ref.ctypes.data, n=8, q=None, nq=0, dim=4, mem=0, radius=1.0, o=off.ctypes.data):
        return L.cilhip_radius_search_nd(0, r, n, q, nq, dim, mem, C.c_float(radius), o, idx.ctypes.data, d2.ctypes.data, 64, C.byref(total))

    for kwargs, code, needle in ((dict(r=None), capi.ERR_INVALID, "ref is NULL"), (dict(o=None), capi.ERR_INVALID, "offsets_out is NULL"), (dict(dim=0), capi.ERR_INVALID, "dim is 0"),
                                 (dict(radius=INF), capi.ERR_INVALID, "not finite"), (dict(radius=float("nan")), capi.ERR_INVALID, "not finite"),
                                 (dict(mem=5), capi.ERR_INVALID, "mem"), (dict(n=2 ** 32 - 16), capi.ERR_INVALID, "2^32 - 16"),
                                 (dict(q=ref.ctypes.data, nq=2 ** 32 - 16), capi.ERR_INVALID, "2^32 - 16"), (dict(dim=17), capi.ERR_UNSUPPORTED, "dim > 16")):
        assert call(**kwargs) == code, kwargs
        assert needle in _err(L) and _err(L).startswith("radius_search_nd: "), (kwargs, _err(L))
        assert (off == 7).all() and (idx == 7).all() and (d2 == 7).all() and total.value == 77


def test_calls_that_need_no_device(hip_lib):
    """n_ref == 0, n_query == 0, a bound that is not positive: padded rows / empty lists, whether or not a device is present"""
    from cilantro_amd import capi, kd_tree

    L = hip_lib
    qry = np.ones((3, 5), np.float32)
    idx = np.full((3, 4), 7, np.uint32); d2 = np.full((3, 4), 7, np.float32); cnt = np.full(3, 7, np.uint32)
    assert L.cilhip_knn_nd(0, None, 0, qry.ctypes.data, 3, 5, 0, 4, C.c_float(INF), idx.ctypes.data, d2.ctypes.data, cnt.ctypes.data) == capi.OK
    assert (idx == capi.NONE_IDX).all() and np.isinf(d2).all() and (cnt == 0).all()
    idx[:] = 7
    for bound in (0.0, -0.0, -1.0, -INF):
        assert L.cilhip_knn_nd(0, qry.ctypes.data, 3, None, 0, 5, 0, 4, C.c_float(bound), idx.ctypes.data, None, None) == capi.OK
        assert (idx == capi.NONE_IDX).all()
    assert L.cilhip_knn_nd(0, qry.ctypes.data, 3, qry.ctypes.data, 0, 5, 0, 4, C.c_float(INF), idx.ctypes.data, None, None) == capi.OK      # no queries
    off = np.full(4, 7, np.uint64)
    total = C.c_size_t(77)
    assert L.cilhip_radius_search_nd(0, None, 0, qry.ctypes.data, 3, 5, 0, C.c_float(1.0), off.ctypes.data, None, None, 0, C.byref(total)) == capi.OK
    assert (off == 0).all() and total.value == 0
    off[:] = 7
    assert L.cilhip_radius_search_nd(0, qry.ctypes.data, 3, None, 0, 5, 0, C.c_float(-2.0), off.ctypes.data, None, None, 0, None) == capi.OK
    assert (off == 0).all()
    # the mirror over the same calls
    import cilantro_amd

    assert cilantro_amd.KDTreeXf is kd_tree.KDTreeXf and cilantro_amd.KDTree2f is kd_tree.KDTree2f and cilantro_amd.KDTree is kd_tree.KDTree
    tree = kd_tree.KDTreeXf(np.zeros((0, 5), np.float32))
    i, d, c = tree.kNNSearch(qry, 2)
    assert tree.dim == 5 and i.shape == (3, 2) and (i == -1).all() and np.isinf(d).all() and (c == 0).all()
    o, i, d = tree.search(qry, kd_tree.RadiusNeighborhoodSpecification(1.0))
    assert o.tolist() == [0, 0, 0, 0] and len(i) == 0 and len(d) == 0
    assert tree.search(qry, kd_tree.KNNInRadiusNeighborhoodSpecification(3, 2.0))[0].shape == (3, 3)
    assert tree.search(qry, kd_tree.KNNNeighborhoodSpecification(1))[0].shape == (3, 1) and tree.nearestNeighborSearch(qry)[0].tolist() == [-1, -1, -1]
    with pytest.raises(capi.CilhipError) as e:
        kd_tree.KDTreeXf(np.zeros((4, 17), np.float32)).kNNSearch(None, 2)
    assert e.value.code == capi.ERR_UNSUPPORTED and "dim > 16" in str(e.value)
    with pytest.raises(ValueError):
        kd_tree.KDTree2f(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        kd_tree.KDTreeXf(np.zeros((4, 3), np.float32)).kNNSearch(np.zeros((2, 4), np.float32), 1)


# ---- knn_nd_host.hpp on its own, and the C++ mirror ----------------------------------------------------------------
def test_host_header_stand_alone_plain_and_sanitized(tmp_path):
    src = os.path.join(HERE, "cpp", "test_knn_nd_host.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_knn_nd_host_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr[-2000:]


def test_cpp_mirror_and_example_compile(tmp_path):
    user = tmp_path / "user.cpp"
    user.write_text("#include <cilantro_hip/kd_tree.hpp>\n"
                    "int main() { float p[4] = {0, 0, 1, 1}; cilantro_hip::KDTree2f t(p, 2); cilantro_hip::KDTreeXf x{cilantro_hip::ConstDataView(p, 4, 1)};\n"
                    "  return (int)t.kNNSearch(p, 1).size() + (int)x.search(x.getPointsMatrixMap(), cilantro_hip::KNNNeighborhoodSpecification(1)).size(); }\n")
    for src in (str(user), os.path.join(ROOT, "examples", "kd_tree.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", src, "-o", str(tmp_path / "out.o")], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    text = open(os.path.join(ROOT, "examples", "kd_tree.cpp")).read()
    for needle in ("kNNInRadiusSearch(ConstPointsView(query), 2, 1.001f)", "KDTreeXf tree4", "Neighbor indices: "):
        assert needle in text, needle
    assert "isualizer" not in text.replace("no visualizer", "")
