"""CPU: the yardstick of the connected-component tests (tests/_cc_refs.py) against itself and against scipy, the preconditions of the
GPU fixtures, the argument rules of the two C entries (they hold without a device), and the g++ build of the C++ mirror and example."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _cc_refs as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def clause_sets(nrm, col, angle):
    """every combination of the three clauses"""
    out = []
    for use_d in (False, True):
        for use_n in (False, True):
            for use_c in (False, True):
                out.append(R.Clauses(max_distance=0.0065 if use_d else None, normals=nrm if use_n else None, max_angle=angle if use_n else None,
                                     angle_inclusive=use_n and not (use_d or use_c), colors=col if use_c else None, color_thresh=0.7 if use_c else None))
    return out


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(0)
    n = 1200
    p = rng.random((n, 3), dtype=np.float32)
    p[:400] *= np.float32(0.3)      # a denser corner: components of many sizes
    nrm = np.array([0, 0, 1], np.float32) + rng.normal(size=(n, 3)).astype(np.float32) * np.float32(0.4)
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[rng.random(n) < 0.5] *= np.float32(-1)
    col = rng.random((n, 3), dtype=np.float32)
    r2 = np.float32(0.09 * 0.09)
    return p, nrm, col, r2, R.brute_lists(p, r2)


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_pair_enumeration_equals_brute_force(small):
    p, _, _, r2, lists = small
    i, j, d2 = R.neighbor_pairs(p, r2)
    got = set(zip(i.tolist(), j.tolist()))
    want = {(a, int(b)) for a in range(len(lists)) for b in lists[a][0] if a > b}
    assert got == want and len(got) > 2000
    assert all(lists[a][0][0] == a for a in range(len(lists)))      # no duplicates: every list starts with its own point


@pytest.mark.parametrize("angle", [0.6, -0.6])
def test_the_two_restatements_agree(small, angle):
    p, nrm, col, r2, lists = small
    n = p.shape[0]
    rng = np.random.default_rng(1)
    seeds = rng.permutation(n)[:150]
    sizes_seen = set()
    for c in clause_sets(nrm, col, np.float32(angle)):
        for kw in ({}, {"min_segment_size": 3}, {"min_segment_size": 2, "max_segment_size": 9}, {"seeds": seeds}, {"seeds": seeds, "min_segment_size": 2, "max_segment_size": 30},
                   {"seeds": seeds[:0]}):
            segs = R.serial_reference(lists, n, c, **kw)
            fast = R.fast_components(p, r2, c, **kw)
            assert same(R.segments_to_arrays(segs, n, order_ties=True), fast), kw
            if "seeds" not in kw:      # all seeds: the stable size sort alone already orders equal sizes by lowest member
                assert same(R.segments_to_arrays(segs, n), fast), kw
            sizes_seen.update(len(s) for s in segs)
    assert len(sizes_seen) > 10


def test_fast_restatement_agrees_with_scipy(small):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import connected_components

    p, nrm, col, r2, _ = small
    n = p.shape[0]
    for c in clause_sets(nrm, col, np.float32(0.6)):
        i, j, d2 = R.neighbor_pairs(p, r2)
        ok = R.similar(c, i, j, d2)
        g = sp.coo_matrix((np.ones(int(ok.sum())), (i[ok], j[ok])), shape=(n, n))
        k, lab = connected_components(g, directed=False)
        low = np.full(k, n, np.int64)
        np.minimum.at(low, lab, np.arange(n))
        labels, offsets, members = R.fast_components(p, r2, c)
        assert len(offsets) - 1 == k
        assert np.array_equal(R.union_find(n, i[ok], j[ok]), low[lab])


def test_chain_reference_equals_the_general_one():
    for kw in ({}, {"gap_at": 1234, "gap": 1.1}):
        p, _ = R.chain(5000, 0.9, 1.0, **kw)
        i, j, _ = R.neighbor_pairs(p, np.float32(1.0))
        assert np.array_equal(R.chain_roots(p, np.float32(1.0)), R.union_find(5000, i, j))


def test_lists_restatement():
    # 0 -> 1, 2 -> 1 (directed): one weak component; 3 alone; 4 <-> 5 masked out; entries >= n are no neighbours
    offsets = [0, 2, 3, 5, 6, 8, 10]
    idx = [0, 1, 1, 2, 1, 3, 4, 5, 5, 4]
    labels, off, mem = R.components_from_lists(6, offsets, idx, skip_first=True)
    assert labels.tolist() == [0, 0, 0, 2, 1, 1] and off.tolist() == [0, 3, 5, 6]
    keep = [1, 1, 1, 1, 1, 1, 1, 0, 1, 0]
    labels, off, mem = R.components_from_lists(6, offsets, idx, keep=keep, skip_first=True)
    assert labels.tolist() == [0, 0, 0, 1, 2, 3]
    labels, off, mem = R.components_from_lists(6, offsets, [0, 1, 1, 2, 1, 3, 4, 0xFFFFFFFF, 5, 9], skip_first=False)
    assert labels.tolist() == [0, 0, 0, 1, 2, 3]


# ---- the preconditions of the GPU fixtures: no decision sits on a threshold ---------------------------------------------------
def test_no_fixture_decision_is_within_4_ulp_of_its_threshold():
    p, nrm, col, flipped = R.downsampled_frame()
    assert p.shape == (15531, 3) and np.isfinite(p).all() and np.isfinite(nrm).all()
    assert np.unique(p, axis=0).shape[0] == p.shape[0]      # no duplicates: the reference's skip of list entry 0 skips the point itself
    for r in (0.02, 0.01):
        for a in (2.0, 5.0):
            near_r, near_a, ones, above = R.near_threshold_counts(p, np.float32(r * r), R.Clauses(normals=nrm, max_angle=R.deg(a)))
            assert (near_r, near_a, ones, above) == (0, 0, 2, 0), (r, a)
            near_r, near_a, _, above = R.near_threshold_counts(p, np.float32(r * r), R.Clauses(normals=flipped, max_angle=-R.deg(a)))
            assert (near_r, near_a, above) == (0, 0, 0), (r, a)
    P, N = R.raw_frame()
    assert np.isfinite(P).all() and np.isfinite(N).all() and np.unique(P, axis=0).shape[0] == P.shape[0]
    near_r, near_a, ones, above = R.near_threshold_counts(P, np.float32(R.RAW_RADIUS ** 2), R.Clauses(normals=N, max_angle=R.deg(5.0)))
    assert (near_r, near_a) == (0, 0) and above > 100      # (the sensor's normals are often a little over-long: the NaN rule is met on real data)
    i, _, _ = R.neighbor_pairs(P, np.float32(R.RAW_RADIUS ** 2))
    assert 20 < 2 * i.size / P.shape[0] < 50


def test_probe_figures_of_the_sensor_frame():
    p, nrm, _, _ = R.downsampled_frame()
    ex = R.Clauses(normals=nrm, max_angle=R.deg(2.0), angle_inclusive=True)
    assert len(R.fast_components(p, np.float32(0.02 ** 2), ex)[1]) - 1 == 5127
    sizes = np.diff(R.fast_components(p, np.float32(0.02 ** 2), ex, min_segment_size=100)[1])
    assert sizes.tolist() == [717, 595, 433, 370, 361, 163, 154, 113]
    sizes = np.diff(R.fast_components(p, np.float32(0.02 ** 2), R.Clauses(normals=nrm, max_angle=R.deg(5.0), angle_inclusive=True), min_segment_size=100)[1])
    assert len(sizes) == 6 and sizes[0] == 9564
    assert np.diff(R.fast_components(p, np.float32(0.02 ** 2))[1]).tolist() == [10548, 2588, 1189, 891, 289, 26]
    sizes = np.diff(R.fast_components(p, np.float32(0.01 ** 2), ex, min_segment_size=10)[1])
    assert len(sizes) == 189 and int((np.diff(sizes) == 0).sum()) == 136


# ---- argument rules: before any device is opened ------------------------------------------------------------------------------
def call(L, n=4, mem=0, radius_sq=1.0, use_normals=0, use_colors=0, normals=False, colors=False, seeds=None, params=True):
    from cilantro_amd import capi

    pts = np.zeros((4, 3), np.float32)
    att = np.zeros((4, 3), np.float32)
    prm = capi.CcParams()
    L.cilhip_cc_default_params(C.byref(prm))
    prm.radius_sq, prm.use_normals, prm.use_colors = radius_sq, use_normals, use_colors
    outs = [np.full(5, 7, np.uint32) for _ in range(3)]
    nseg = C.c_size_t(77)
    s = None if seeds is None else np.asarray(seeds, np.uint32)
    rc = L.cilhip_connected_components3f(0, pts.ctypes.data, att.ctypes.data if normals else None, att.ctypes.data if colors else None, n, mem,
                                         C.byref(prm) if params else None, None if s is None else s.ctypes.data, 0 if s is None else s.size,
                                         outs[0].ctypes.data, outs[1].ctypes.data, outs[2].ctypes.data, C.byref(nseg))
    untouched = all((o == 7).all() for o in outs) and nseg.value == 77
    return rc, untouched, L.cilhip_last_error(None).decode()


def test_refused_input_needs_no_device(hip_lib):
    from cilantro_amd import capi

    L = hip_lib
    for kw, word in (({"use_normals": 1}, "normals"), ({"use_colors": 1}, "colours"), ({"use_normals": 1, "colors": True}, "normals"), ({"seeds": [0, 4]}, "seed"),
                     ({"n": 1 << 32}, "2^32"), ({"mem": 2}, "mem"), ({"radius_sq": float("nan")}, "radius_sq"), ({"radius_sq": float("inf")}, "radius_sq"),
                     ({"params": False}, "params")):
        rc, untouched, err = call(L, **kw)
        assert rc == capi.ERR_INVALID and untouched and word in err and err.startswith("connected_components"), (kw, err)
    # n == 0: answered without a device
    prm = capi.CcParams()
    L.cilhip_cc_default_params(C.byref(prm))
    assert (prm.min_segment_size, prm.max_segment_size, prm.use_distance, prm.use_normals, prm.use_colors) == (1, (1 << 64) - 1, 0, 0, 0)
    nseg = C.c_size_t(77)
    off = np.full(1, 7, np.uint32)
    assert L.cilhip_connected_components3f(0, None, None, None, 0, 0, C.byref(prm), None, 0, None, off.ctypes.data, None, C.byref(nseg)) == capi.OK
    assert nseg.value == 0 and off[0] == 0
    # the lists entry: the shared rules, and a seed list over directed lists
    offsets, idx, lab = np.array([0, 1, 2], np.uint64), np.array([1, 0], np.uint32), np.full(2, 7, np.uint32)
    seeds = np.array([1], np.uint32)
    lists = lambda n, mem, symmetric, s: L.cilhip_connected_components_lists(0, n, offsets.ctypes.data, idx.ctypes.data, None, 2, 0, symmetric, mem, 1, 10,      # noqa: E731
                                                                             None if s is None else s.ctypes.data, 0 if s is None else s.size, lab.ctypes.data, None, None, C.byref(nseg))
    nseg.value = 77
    assert lists(2, 0, 0, seeds) == capi.ERR_UNSUPPORTED and "directed" in L.cilhip_last_error(None).decode()
    assert lists(2, 3, 1, None) == capi.ERR_INVALID and lists(1 << 32, 0, 1, None) == capi.ERR_INVALID
    assert lists(2, 0, 1, np.array([2], np.uint32)) == capi.ERR_INVALID and "seed" in L.cilhip_last_error(None).decode()
    assert (lab == 7).all() and nseg.value == 77
    assert lists(0, 0, 1, None) == capi.OK and nseg.value == 0
    import torch

    if not torch.cuda.is_available():      # a valid call fails loudly: there is no CPU path
        rc, _, err = call(L)
        assert rc == capi.ERR_NO_DEVICE and "no CPU path" in err
        from cilantro_amd import clustering

        with pytest.raises(capi.CilhipError):
            clustering.ConnectedComponentExtraction3f(np.zeros((4, 3), np.float32)).segment(clustering.RadiusNeighborhoodSpecification(1.0))


# ---- the C++ mirror and the example compile with g++ ----------------------------------------------------------------------------
def build_cpp(src, name):
    """one translation unit against the public headers and the library -> the binary's path"""
    from cilantro_amd import build, capi

    if not os.path.exists(capi.LIB_PATH):
        build.build()
    out_dir = os.path.join(HERE, "cpp", "bin")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name)
    lib = os.path.join(ROOT, "cilantro_amd", "lib")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), src, "-o", out, "-L" + lib, "-lcilantro_hip", "-Wl,-rpath," + lib,
           "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def test_cpp_mirror_and_example_compile(tmp_path):
    exe = build_cpp(os.path.join(HERE, "cpp", "test_components.cpp"), "test_components")
    build_cpp(os.path.join(ROOT, "examples", "connected_component_extraction.cpp"), "example_connected_component_extraction")
    # the host half of the mirror: removeInvalidData and its siblings compact on the host, no device needed
    r = subprocess.run([exe, "host"], capture_output=True, text=True)
    assert r.returncode == 0 and "host OK" in r.stdout, r.stdout + r.stderr
    src = open(os.path.join(ROOT, "examples", "connected_component_extraction.cpp")).read()
    for needle in ("gridDownsample(0.005f)", "removeInvalidData()", "ConnectedComponentExtraction3f", "NormalsProximityEvaluator"):
        assert needle in src, needle
