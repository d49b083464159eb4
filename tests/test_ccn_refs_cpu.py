"""CPU: the yardstick of the N-D connected-component tests (tests/_ccn_refs.py) against scipy and against the 3-D yardstick, the margins of
the fixtures the GPU test shares (so that it needs no exclusions), R and the prune rule in numpy, the argument rules of
cilhip_connected_components_nd (they hold without a device), csrc/components_nd_host.hpp stand-alone (plainly and under ASan / UBSan), the
g++ build of the C++ mirror and the example, and the symbols."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import _cc_refs as R3
import _ccn_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", range(1, 17))
def test_partition_equals_scipy_on_the_same_edges(dim):
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    p, r2 = R.blob_fixture(dim)
    n = p.shape[0]
    i, j, d2 = R.cached_pairs(p, r2)
    assert p.shape == (1500, dim) and i.size > 0 and (i > j).all() and (d2 < r2).all()
    root = R.roots(p, r2)
    ncomp, lab = connected_components(coo_matrix((np.ones(i.size), (i, j)), shape=(n, n)), directed=False)
    assert ncomp == len(np.unique(root)) and 1 < ncomp < n      # neither one blob nor dust
    low = np.full(ncomp, n, np.int64)      # scipy's labels -> lowest member
    np.minimum.at(low, lab, np.arange(n))
    assert np.array_equal(low[lab], root)
    labels, offsets, members = R.components(p, r2)
    sizes = np.diff(offsets)
    assert offsets[-1] == n and (np.diff(sizes) <= 0).all() and sizes[0] > 1 and np.array_equal(np.sort(members), np.arange(n))


def test_at_dim_3_the_yardstick_is_the_3d_yardstick_under_all_eight_evaluators():
    p, nrm, col, flipped = R3.downsampled_frame()
    p, nrm, col, flipped = p[:4000], nrm[:4000], col[:4000], flipped[:4000]
    r2 = F32(0.0075 * 0.0075)
    seen = set()
    for name, _, cl in R3.evaluator_cases(nrm, flipped, col):
        want = R3.fast_components(p, r2, cl)
        got = R.components(p, r2, cl)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), name
        seen.add(len(want[1]))
    assert len(seen) >= 4      # the clauses change the result
    i = np.arange(1, 4000)
    assert R.dot_fold(nrm[i], nrm[i - 1]).tobytes() == R3.dot_pinned(nrm[i], nrm[i - 1]).tobytes()      # x x' + (y y' + z z')


def test_the_fold_of_the_dot_product_is_from_the_last_axis():
    a = np.array([[1e8, 1.0, -1e8, 3.0]], F32)
    b = np.ones((1, 4), F32)
    assert R.dot_fold(a, b)[0] == F32(1e8) + (F32(1.0) + (F32(-1e8) + F32(3.0)))      # = 0: 1e8 + (1 + (-1e8 + 3)) absorbs the small terms
    assert R.dot_fold(a, b)[0] != ((F32(1e8) + F32(1.0)) + F32(-1e8)) + F32(3.0)      # the ascending order gives 3


# ---- the fixtures' margins: the GPU test compares exactly and excludes nothing ---------------------------------------------------------
def random_fixtures():
    out = [(f"blobs_{d}",) + R.blob_fixture(d) + (None,) for d in range(1, 17)]
    out += [(f"size_{n}_{d}",) + R.size_fixture(n, d) + (None,) for d in R.SIZE_DIMS for n in R.SIZES if n > 2]
    out.append(("duplicates",) + R.duplicates_fixture() + (None,))
    p, r2, _ = R.nonfinite_fixture()
    out.append(("nonfinite", p, r2, None))
    p, r2, _ = R.two_far_blobs()
    out.append(("two_far_blobs", p, r2, None))
    for d in (2, 6):
        p, r2 = R.evaluator_fixture(d)[:2]
        out += [(f"eval_{d}_{k}_{name}", p, r2, cl) for k, (name, _, cl) in enumerate(R.evaluator_cases(d))]
    return out


def test_no_random_fixture_decides_within_4_ulp_of_a_threshold():
    for name, p, r2, cl in random_fixtures():
        m = R.margins(p, r2, cl)
        assert m == {"radius": 0, "distance": 0, "colour": 0, "angle": 0}, (name, m)


def test_the_lattice_and_the_chain_sit_on_their_thresholds_on_purpose():
    p, r2 = R.lattice_fixture()
    i, j, d2 = R.pairs(p, F32(2.5))
    assert r2 == 2.0 and (d2 == 2.0).sum() > 100 and (d2 == 1.0).sum() > 100      # the d2 = 2 shell is ON the threshold ...
    k, l, e2 = R.cached_pairs(p, r2)
    assert (e2 == 1.0).all() and e2.size == (d2 == 1.0).sum()      # ... and strict < leaves it out
    looser = R3.union_find(len(p), i[d2 <= 2.0], j[d2 <= 2.0])
    assert len(np.unique(looser)) < len(np.unique(R.roots(p, r2)))      # <= would give another partition
    c, pos = R.chain_fixture()
    assert c.shape == (3 * R.TILE + 5, 5)
    order = np.argsort(pos)
    from _knn_nd_refs import d2_matrix

    step = np.array([d2_matrix(c[order[k:k + 1]], c[order[k + 1:k + 2]])[0, 0] for k in range(len(c) - 1)])
    assert (step == F32(0.3125)).all() and F32(0.3125) < R.CHAIN_R2 < F32(1.25)
    assert len(np.unique(R.roots(c, R.CHAIN_R2))) == 1
    g, _ = R.chain_fixture(gap_at=400)
    assert np.bincount(R.roots(g, R.CHAIN_R2))[[0, 401]].tolist() == [401, len(g) - 401]
    s, spos = R.chain_fixture(shuffled=True)
    assert not np.array_equal(spos, np.arange(len(s))) and (R.roots(s, R.CHAIN_R2) == 0).all()      # the root is the lowest ORIGINAL index


def test_fixture_properties_the_gpu_test_relies_on():
    p, r2, rows = R.nonfinite_fixture()
    root = R.roots(p, r2)
    assert (root[rows] == rows).all() and (np.bincount(root)[rows] == 1).all()      # NaN, +-inf and 1e20 rows are singletons
    assert np.isfinite(p[rows[[3, 4, 6, 8]]]).all(axis=1).all() and (np.abs(p[rows[[3, 4, 6, 8]]]).max(axis=1) >= 1e20).all()      # ... the 1e20 rows being finite rows whose d2 overflows
    assert len(np.unique(root)) < len(p) - 100
    q, q2 = R.duplicates_fixture()
    lab, off, mem = R.components(q, q2)
    sizes = np.diff(off)
    assert (sizes == 2).sum() >= 20 and (sizes == 3).sum() >= 10 and (sizes == 1).sum() > 100
    for d in (2, 6):
        p, r2, nrm, flipped, col = R.evaluator_fixture(d)
        counts = [len(R.components(p, r2, cl)[1]) - 1 for _, _, cl in R.evaluator_cases(d)]
        assert len(set(counts)) >= 6, counts      # every clause changes the result
        assert R.dot_fold(nrm[10], nrm[11]) > 1 and np.isnan(R.pair_angle(nrm, np.array([10]), np.array([11]))[0]) and (p[10] == p[11]).all()
        cl = R.Clauses(normals=nrm, max_angle=R3.deg(20.0), angle_inclusive=True)
        i, j, _ = R.cached_pairs(p, r2)
        pair = (i == 11) & (j == 10)
        assert pair.sum() == 1 and not R.similar(cl, i[pair], j[pair], np.zeros(1, F32))[0]      # inside the radius, a dot above 1: not similar
    p, r2, axis = R.two_far_blobs()
    assert R.pick_axis(p) == axis and len(np.unique(R.roots(p, r2))) >= 2


# ---- R and the prune rule -----------------------------------------------------------------------------------------------------------
def test_R_is_the_smallest_float_whose_square_reaches_radius_sq():
    rng = np.random.default_rng(2)
    bits = rng.integers(1, 0x7F7FFFFF, 9990, dtype=np.int64).astype(np.uint32)
    tiny, fmax = np.finfo(F32).smallest_subnormal, np.finfo(F32).max
    radii = np.concatenate([bits.view(F32), np.array([tiny, 2 * tiny, np.finfo(F32).tiny, 1.0, 2.0, 4.0, 0.32, 1e30, fmax, np.nextafter(F32(1), F32(2))], F32)])
    assert len(radii) == 10000
    with np.errstate(over="ignore", under="ignore"):
        for r2 in radii[::1]:
            Rr = R.prune_radius(r2)
            assert Rr > 0 and Rr * Rr >= r2, (r2, Rr)
            prev = np.nextafter(Rr, F32(0))
            assert prev * prev < r2, (r2, Rr)
    assert R.prune_radius(F32(4)) == 2 and R.prune_radius(np.nextafter(F32(4), F32(5))) == np.nextafter(F32(2), F32(3))
    assert R.prune_radius(F32(0)) == tiny      # fl(R * R) = 0 >= 0 for every R: the smallest positive float (radius_sq <= 0 never reaches the prune: every point is a singleton)


@pytest.mark.parametrize("dim", [1, 2, 5, 16])
def test_no_skipped_tile_pair_holds_an_edge(dim):
    from _knn_nd_refs import d2_matrix

    rng = np.random.default_rng(40 + dim)
    skipped_total = 0
    for tile, n, scale in ((8, 300, 1.0), (16, 500, 20.0), (8, 257, 1e-3)):
        p = (rng.standard_normal((n, dim)) * np.linspace(1.0, 3.0, dim)[None, :] * scale).astype(F32)
        p[rng.integers(0, n, 5), rng.integers(0, dim, 5)] = np.nan      # dropped rows
        r2 = R.radius_for(p[np.isfinite(p).all(axis=1)], 0.7)
        Rr = R.prune_radius(r2)
        axis = R.pick_axis(p)
        order = R.sweep_order(p, axis)
        s = p[order]
        assert (np.diff(s[:, axis]) >= 0).all() and len(order) == np.isfinite(p).all(axis=1).sum()
        first = R.first_columns(s[:, axis], Rr, tile)
        assert (np.diff(first) >= 0).all() and (first <= np.arange(len(first))).all()
        d = d2_matrix(s, s)
        for t in range(len(first)):
            block = d[t * tile:(t + 1) * tile, :first[t] * tile]
            assert not (block < r2).any(), (dim, tile, t)
            skipped_total += int(first[t])
    assert skipped_total > 50      # the rule skips something on these clouds


def test_keys_sort_like_floats():
    rng = np.random.default_rng(3)
    v = np.concatenate([rng.standard_normal(1000).astype(F32) * F32(1e10), np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45], F32)])
    k = R.key(v)
    order = np.argsort(k, kind="stable")
    assert (np.diff(v[order]) >= 0).all() and k[v.tolist().index(0.0)] > k[len(v) - 5] and (k < 0xFFFFFFFF).all()
    src = open(os.path.join(ROOT, "cilantro_amd", "csrc", "components_nd_host.hpp")).read()
    assert f"constexpr size_t CCN_TILE = {R.TILE};" in src


# ---- argument rules: before any device is opened ------------------------------------------------------------------------------------
def call(L, n=4, dim=5, points=True, normals=False, rgb=False, mem=0, params=True, form=0, seeds=None, n_seeds=0, labels=True, nseg=True, **fields):
    from cilantro_amd import capi

    pts = np.zeros((4, 20), np.float32)
    prm = capi.CcParams()
    L.cilhip_cc_default_params(C.byref(prm))
    prm.radius_sq = 1.0
    for k, v in fields.items():
        setattr(prm, k, v)
    u = [np.full(6, 7, np.uint32) for _ in range(3)]
    ns = C.c_size_t(77)
    sd = None if seeds is None else np.asarray(seeds, np.uint32)
    rc = L.cilhip_connected_components_nd(0, pts.ctypes.data if points else None, pts.ctypes.data if normals else None, pts.ctypes.data if rgb else None, n, dim, mem,
                                          C.byref(prm) if params else None, form, None if sd is None else sd.ctypes.data, n_seeds, u[0].ctypes.data if labels else None,
                                          u[1].ctypes.data, u[2].ctypes.data, C.byref(ns) if nseg else None)
    untouched = all((a == 7).all() for a in u) and ns.value == 77
    return rc, untouched, L.cilhip_last_error(None).decode()


def test_refused_input_needs_no_device(hip_lib):
    from cilantro_amd import capi, clustering

    L = hip_lib
    nan, inf = float("nan"), float("inf")
    rows = [({"dim": 0}, "dim is 0"), ({"form": 3}, "form"), ({"form": -1}, "form"), ({"n": 2 ** 32 - 16}, "n must be below 2^32 - 16"), ({"n": 2 ** 32}, "n must be below 2^32 - 16"),
            ({"points": False}, "points is null"), ({"n_seeds": 3}, "seed array"), ({"seeds": [0, 4], "n_seeds": 2}, "seed index"),
            ({"radius_sq": nan}, "radius_sq"), ({"radius_sq": inf}, "radius_sq"), ({"radius_sq": -inf}, "radius_sq"),
            ({"use_normals": 1}, "normals clause"), ({"use_colors": 1}, "colours clause"), ({"use_normals": 1, "rgb": True}, "normals clause"),
            ({"mem": 2}, "mem"), ({"mem": -1}, "mem"), ({"params": False}, "params is null"), ({"labels": False}, "labels_out is null"), ({"nseg": False}, "n_segments_out is null")]
    for kw, word in rows:
        rc, untouched, err = call(L, **kw)
        assert rc == capi.ERR_INVALID and untouched and word in err and err.startswith("connected_components_nd: "), (kw, rc, err)
    for dim in (17, 1000):
        rc, untouched, err = call(L, dim=dim)
        assert rc == capi.ERR_UNSUPPORTED and untouched and "dim > 16" in err and err.startswith("connected_components_nd: "), (dim, rc, err)
    # no point at all: answered without a device
    prm = capi.CcParams()
    L.cilhip_cc_default_params(C.byref(prm))
    prm.radius_sq = 1.0
    ns, off = C.c_size_t(77), np.full(1, 7, np.uint32)
    assert L.cilhip_connected_components_nd(0, None, None, None, 0, 6, 0, C.byref(prm), 0, None, 0, None, off.ctypes.data, None, C.byref(ns)) == capi.OK
    assert ns.value == 0 and off[0] == 0
    lab, offs, mem = clustering.connected_components_nd(np.zeros((0, 9), np.float32), 1.0)
    assert lab.shape == (0,) and offs.tolist() == [0] and mem.shape == (0,)
    cce = clustering.ConnectedComponentExtractionXf(np.zeros((0, 4), np.float32)).segment(clustering.RadiusNeighborhoodSpecification(1.0))
    assert cce.getNumberOfClusters() == 0 and cce.getNumberOfPoints() == 0 and cce.dim == 4 and cce.getLastStats() == {}
    with pytest.raises(capi.CilhipError) as e:
        clustering.ConnectedComponentExtractionXf(np.zeros((4, 17), np.float32)).segment(clustering.RadiusNeighborhoodSpecification(1.0))
    assert e.value.code == capi.ERR_UNSUPPORTED and "dim > 16" in str(e.value)
    with pytest.raises(ValueError):
        clustering.ConnectedComponentExtraction2f(np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError):
        clustering.ConnectedComponentExtractionXf(np.zeros((4, 3), np.float32), dim=4)
    with pytest.raises(ValueError):      # normals are n x dim
        clustering.connected_components_nd(np.zeros((4, 5), np.float32), 1.0, clustering.NormalsProximityEvaluator(np.zeros((4, 3), np.float32), 0.1))
    with pytest.raises(TypeError) as te:      # a non-radius neighbourhood: the same pointer as in 3-D
        clustering.ConnectedComponentExtraction2f(np.zeros((4, 2), np.float32)).segment(object())
    assert "connected_components_from_lists" in str(te.value)
    with pytest.raises(TypeError) as te3:
        clustering.ConnectedComponentExtraction3f(np.zeros((4, 3), np.float32)).segment(object())
    assert str(te.value) == str(te3.value)
    import torch

    if not torch.cuda.is_available():      # a valid call fails loudly: there is no CPU path
        rc, _, err = call(L)
        assert rc == capi.ERR_NO_DEVICE and "no CPU path" in err
        with pytest.raises(capi.CilhipError):
            clustering.ConnectedComponentExtraction2f(np.zeros((4, 2), np.float32)).segment(clustering.RadiusNeighborhoodSpecification(1.0))


def test_symbols_sources_and_exports():
    import cilantro_amd
    from cilantro_amd import build, capi, clustering

    header = open(os.path.join(ROOT, "include", "cilantro_hip", "c_api.h")).read()
    for sym in ("cilhip_connected_components_nd", "cilhip_ccn_last_stats"):
        assert sym in capi.SYMBOLS and re.search(r"\bint " + sym + r"\(", header), sym
    assert "cilhip_ccn_set_pair_cap" in capi.SYMBOLS and "void cilhip_ccn_set_pair_cap(size_t max_pairs_per_launch);" in header
    assert "typedef struct cilhip_ccn_stats { int form_used; size_t axis, tiles_total, tiles_tested, launches; double prep_ms, hook_ms, finish_ms; } cilhip_ccn_stats;" in header
    assert [f[0] for f in capi.CcnStats._fields_] == ["form_used", "axis", "tiles_total", "tiles_tested", "launches", "prep_ms", "hook_ms", "finish_ms"]
    for rule in ("C1 graph", "C2 clauses", "C3 output", "C4 repeatable", "C5 refusals", "connected_component_extraction.hpp:162-265, :394-457", "common_pair_evaluators.hpp:92-259"):
        assert rule in header, rule
    assert "components_nd.hip" in build.SOURCES and "components_nd_host.hpp" in build.HEADERS and "components_device.hpp" in build.HEADERS
    csrc = os.path.join(ROOT, "cilantro_amd", "csrc")
    host = open(os.path.join(csrc, "components_nd_host.hpp")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host      # plain C++
    # the union-find and the tail are written once, and both units include them
    shared = open(os.path.join(csrc, "components_device.hpp")).read()
    for unit in ("components.hip", "components_nd.hip"):
        src = open(os.path.join(csrc, unit)).read()
        assert '#include "components_device.hpp"' in src, unit
        for name in ("uint32_t cc_find(", "uint32_t cc_unite(", "int cc_finish(", "void k_cc_flatten(", "struct CcOut"):
            assert name not in src and name in shared, (unit, name)
    unit = open(os.path.join(csrc, "components_nd.hip")).read()
    assert "ND_DISPATCH(dim, CCN_RUN)" in unit and "NdQuery<DIM> q;" in unit and "atomicAdd(float" not in unit
    for name in ("ConnectedComponentExtraction2f", "ConnectedComponentExtractionXf", "connected_components_nd"):
        assert getattr(cilantro_amd, name) is getattr(clustering, name) and name in cilantro_amd.__all__
    assert issubclass(clustering.ConnectedComponentExtraction2f, clustering.ConnectedComponentExtractionXf)
    assert issubclass(clustering.ConnectedComponentExtractionXf, clustering.ConnectedComponentExtraction3f)
    for method in ("segment", "getPointToClusterIndexMap", "getNumberOfClusters", "getNumberOfPoints", "getClusterToPointIndicesMap", "getLabeledPointIndices", "getUnlabeledPointIndices"):
        assert callable(getattr(clustering.ConnectedComponentExtractionXf, method))


# ---- components_nd_host.hpp on its own, the C++ mirror and the example ----------------------------------------------------------------
def test_host_header_stand_alone_plain_and_sanitized(tmp_path):
    src = os.path.join(HERE, "cpp", "test_components_nd_host.cpp")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("test_components_nd_host_" + name))
        r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + [src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr[-2000:]


def test_cpp_mirror_and_example_compile():
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_components_nd.cpp"), "test_components_nd")
    build_cpp(os.path.join(ROOT, "examples", "connected_component_extraction_nd.cpp"), "example_connected_component_extraction_nd")
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "connected_component_extraction_nd.cpp")).read()
    for needle in ("ConnectedComponentExtractionXf<> cce{ConstDataView(features, dim)}", "PointsNormalsProximityEvaluator", "getClusterToPointIndicesMap", "getLastStats"):
        assert needle in src, needle
    mirror = open(os.path.join(ROOT, "include", "cilantro_hip", "clustering.hpp")).read()
    assert "class ConnectedComponentExtractionXf" in mirror and "class ConnectedComponentExtraction2f" in mirror and "class ConnectedComponentExtraction3f" in mirror
