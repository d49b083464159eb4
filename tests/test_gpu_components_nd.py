"""GPU: cilhip_connected_components_nd against the yardstick of tests/_ccn_refs.py -- labels, offsets, members and the
segment count compared exactly, in forms 1 (the exhaustive triangle) and 2 (sweep and prune).  No case is excluded and no tolerance is
used: tests/test_ccn_refs_cpu.py asserts that no random fixture decides within 4 ulp of a threshold, and the lattice and the chain sit on
their thresholds on purpose."""
import numpy as np
import pytest

import _cc_refs as R3
import _ccn_refs as R

pytestmark = pytest.mark.gpu
F32 = np.float32
T = R.TILE


def evaluator_of(cl):
    """a Clauses record as the evaluator description the Python mirror takes"""
    from cilantro_amd import clustering

    ev = clustering.AlwaysTrueEvaluator()
    if cl is not None:
        ev.normals, ev.colors, ev.max_distance, ev.max_angle, ev.color_thresh, ev.angle_inclusive = cl.normals, cl.colors, cl.max_distance, cl.max_angle, cl.color_thresh, cl.angle_inclusive
    return ev


def run(p, r2, cl=None, form=0, seeds=None, min_segment_size=1, max_segment_size=None, stats=None, on_device=False):
    from cilantro_amd import clustering

    ev = evaluator_of(cl)
    if on_device:
        import torch

        p = torch.from_numpy(p).cuda()
        ev.normals = None if ev.normals is None else torch.from_numpy(ev.normals).cuda()
        ev.colors = None if ev.colors is None else torch.from_numpy(ev.colors).cuda()
    out = clustering.connected_components_nd(p, float(r2), ev, min_segment_size, clustering.SIZE_MAX if max_segment_size is None else max_segment_size, seeds, form, 0, stats)
    return tuple(o.cpu().numpy() if on_device else o for o in out)


def same(got, want, what=""):
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b), (what, ("labels", "offsets", "members")[k], int((a != b).sum()) if a.shape == b.shape else (a.shape, b.shape))


def both_forms(p, r2, cl=None, what="", **kw):
    want = R.components(p, r2, cl, **kw)
    for form in (1, 2):
        st = {}
        same(run(p, r2, cl, form, stats=st, **kw), want, (what, "form", form))
        assert st["form_used"] == form
    return want


@pytest.mark.parametrize("dim", range(1, 17))
def test_every_dimension(dim):
    p, r2 = R.blob_fixture(dim)
    want = both_forms(p, r2, what=dim)
    assert 2 < len(want[1]) - 1 < 1500 and want[1][1] > 30      # several segments, large ones among them


@pytest.mark.parametrize("dim", R.SIZE_DIMS)
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes_around_the_tile(n, dim):
    p, r2 = R.size_fixture(n, dim)
    want = both_forms(p, r2, what=(n, dim))
    assert want[0].shape == (n,) and (n != 2 or want[1].tolist() == [0, 2])


def test_a_chain_across_every_tile_pair():
    p, _ = R.chain_fixture()
    want = both_forms(p, R.CHAIN_R2, what="chain")
    assert want[1].tolist() == [0, 3 * T + 5]      # one component
    g, _ = R.chain_fixture(gap_at=400)
    want = both_forms(g, R.CHAIN_R2, what="chain with a gap")
    assert want[1].tolist() == [0, 401, 3 * T + 5]      # two; the larger one (positions 0 .. 400) first
    s, pos = R.chain_fixture(shuffled=True)
    want = both_forms(s, R.CHAIN_R2, what="shuffled chain")
    assert want[1].tolist() == [0, 3 * T + 5] and want[2][0] == 0 and np.array_equal(want[2], np.arange(3 * T + 5))
    sg, pos = R.chain_fixture(gap_at=400, shuffled=True)
    want = both_forms(sg, R.CHAIN_R2, what="shuffled chain with a gap")
    low = [int(np.nonzero(pos <= 400)[0].min()), int(np.nonzero(pos > 400)[0].min())]      # each part's lowest ORIGINAL index leads its list
    assert sorted(want[2][want[1][:2]].tolist()) == sorted(low)


def test_a_lattice_with_the_radius_on_a_shell():
    p, r2 = R.lattice_fixture()
    want = both_forms(p, r2, what="lattice")
    assert 1 < len(want[1]) - 1 < len(p)
    same(run(p, np.nextafter(F32(2.0), F32(3.0)), form=2), R.components(p, np.nextafter(F32(2.0), F32(3.0))), "one ulp above the shell")


def test_doubled_and_tripled_rows():
    p, r2 = R.duplicates_fixture()
    both_forms(p, r2, what="duplicates")


def test_non_finite_and_huge_rows_are_singletons():
    p, r2, rows = R.nonfinite_fixture()
    want = both_forms(p, r2, what="nonfinite")
    for form in (1, 2):
        labels, offsets, members = run(p, r2, form=form)
        sizes = np.diff(offsets)
        assert (sizes[labels[rows]] == 1).all() and np.array_equal(np.sort(members), np.arange(len(p)))      # none lost, none misplaced
    # nothing but non-finite rows, and one finite row among them
    q = np.full((300, 6), np.nan, F32)
    q[7] = 1.0
    both_forms(q, F32(4.0), what="all NaN but one")
    both_forms(np.full((5, 3), np.inf, F32), F32(4.0), what="all inf")


@pytest.mark.parametrize("dim", [2, 6])
@pytest.mark.parametrize("case", range(12))
def test_all_eight_evaluators(case, dim):
    from cilantro_amd import clustering

    p, r2 = R.evaluator_fixture(dim)[:2]
    name, args, cl = R.evaluator_cases(dim)[case]
    want = both_forms(p, r2, cl, what=(name, dim))
    cce = clustering.ConnectedComponentExtractionXf(p, dim).segment(clustering.RadiusNeighborhoodSpecification(float(r2)), getattr(clustering, name)(*args))      # the class itself
    assert np.array_equal(cce.getPointToClusterIndexMap(), want[0]) and cce.getNumberOfClusters() == len(want[1]) - 1


def test_radius_not_positive_makes_singletons():
    p, _ = R.blob_fixture(4)
    for r2 in (0.0, -1.0):
        for form in (0, 1, 2):
            labels, offsets, members = run(p, r2, form=form)
            assert np.array_equal(labels, np.arange(1500)) and np.array_equal(offsets, np.arange(1501)) and np.array_equal(members, np.arange(1500))


def test_seeds_and_size_limits():
    p, r2 = R.blob_fixture(6)
    full = R.components(p, r2)
    sizes = np.diff(full[1])
    assert (sizes == 1).sum() > 10 and (sizes[1:] == sizes[:-1]).any()      # equal sizes exist: ordered by lowest member
    for kw in ({"seeds": None}, {"seeds": np.array([0, 5, 1499, 5])}, {"seeds": np.zeros(0, np.int64)}, {"seeds": full[2][full[1][1]:full[1][1] + 1]},
               {"min_segment_size": 2}, {"max_segment_size": int(sizes[0]) - 1}, {"min_segment_size": 2, "max_segment_size": int(sizes[1])},
               {"min_segment_size": 3, "seeds": np.arange(0, 1500, 7)}, {"min_segment_size": 1500}):
        want = both_forms(p, r2, what=str(kw), **kw)
        if kw.get("seeds") is not None and len(kw["seeds"]) == 0:
            assert len(want[1]) == 1 and (want[0] == 0).all()
    assert len(R.components(p, r2, min_segment_size=2)[1]) < len(full[1]) and len(R.components(p, r2, max_segment_size=int(sizes[0]) - 1)[1]) == len(full[1]) - 1


def test_host_and_device_memory_agree():
    for dim in (2, 6):
        p, r2 = R.evaluator_fixture(dim)[:2]
        _, _, cl = R.evaluator_cases(dim)[7]      # distance + normals + colours
        want = R.components(p, r2, cl)
        for form in (1, 2):
            same(run(p, r2, cl, form, on_device=True), want, ("device", dim, form))
            same(run(p, r2, cl, form, on_device=False), want, ("host", dim, form))


def test_two_runs_and_all_forms_agree_on_every_word():
    for dim in (3, 9, 16):
        p, r2 = R.blob_fixture(dim)
        outs = [run(p, r2, form=f) for f in (1, 1, 2, 2, 0)]
        for o in outs[1:]:
            same(o, outs[0], dim)
    # form 0: the exhaustive triangle below the measured crossover (CCN_FORM2_MIN_POINTS = 65536), the sweep from there up
    st = {}
    run(R.blob_fixture(5)[0], R.blob_fixture(5)[1], form=0, stats=st)
    assert st["form_used"] == 1
    rng = np.random.default_rng(77)
    big = rng.random((65536, 2), dtype=F32)
    outs = []
    for n, want_form in ((65535, 1), (65536, 2)):
        outs = [run(big[:n], 1.5e-5, form=f, stats=st) for f in (1, 2, 0)]
        assert st["form_used"] == want_form, n
        same(outs[1], outs[0], n)
        same(outs[2], outs[0], n)
    assert 10 < len(outs[0][1]) - 1 < 65536


def test_dim_3_equals_the_3d_entry_under_every_clause():
    from cilantro_amd import clustering

    p, nrm, col, flipped = R3.downsampled_frame()
    p, nrm, col, flipped = (np.ascontiguousarray(a[:4000]) for a in (p, nrm, col, flipped))
    r2 = float(F32(0.0075 * 0.0075))
    for name, args, cl in R3.evaluator_cases(nrm, flipped, col):
        ev = getattr(clustering, name)(*args)
        want = clustering.connected_components(p, r2, ev)
        for form in (1, 2):
            same(clustering.connected_components_nd(p, r2, ev, form=form), want, (name, form))
        want = clustering.connected_components(p, r2, ev, 3, 500, np.arange(0, 4000, 3))
        same(clustering.connected_components_nd(p, r2, ev, 3, 500, np.arange(0, 4000, 3), 2), want, (name, "seeds and limits"))


def test_stats_say_what_ran():
    p, r2 = R.size_fixture(4097, 6)
    st = {}
    want = R.components(p, r2)
    same(run(p, r2, form=1, stats=st), want)
    tiles = (4097 + T - 1) // T
    assert st["form_used"] == 1 and st["tiles_total"] == tiles * (tiles + 1) // 2 == st["tiles_tested"] and st["launches"] == 1
    assert st["prep_ms"] >= 0 and st["hook_ms"] > 0 and st["finish_ms"] > 0
    same(run(p, r2, form=2, stats=st), want)
    assert st["form_used"] == 2 and st["tiles_total"] == tiles * (tiles + 1) // 2 and 0 < st["tiles_tested"] <= st["tiles_total"] and st["axis"] == R.pick_axis(p)
    # two blobs far apart along one axis: the sweep picks that axis and does not test the tile pairs between them
    q, q2, axis = R.two_far_blobs()
    same(run(q, q2, form=2, stats=st), R.components(q, q2))
    assert st["axis"] == axis and st["tiles_tested"] < st["tiles_total"] and st["tiles_total"] == 15
    order = R.sweep_order(q, axis)
    first = R.first_columns(q[order, axis], R.prune_radius(q2))
    assert st["tiles_tested"] == int((np.arange(len(first)) - first + 1).sum())      # the plan is the rule's, tile pair for tile pair


def test_a_plan_cut_into_several_launches_gives_the_same_words():
    from cilantro_amd import capi

    L = capi.load()
    p, r2 = R.size_fixture(4097, 6)
    _, _, cl = R.evaluator_cases(6)[5]
    q, q2 = R.evaluator_fixture(6)[:2]
    try:
        L.cilhip_ccn_set_pair_cap(3 * T * T)      # three tile pairs per launch
        for form in (1, 2):
            st = {}
            same(run(p, r2, form=form, stats=st), R.components(p, r2), ("cut", form))
            assert st["launches"] == (st["tiles_tested"] + 2) // 3 > 1
            same(run(q, q2, cl, form, stats=st), R.components(q, q2, cl), ("cut, clauses", form))
            assert st["launches"] > 1
        L.cilhip_ccn_set_pair_cap(1)      # one tile pair per launch
        st = {}
        same(run(q, q2, cl, 2, stats=st), R.components(q, q2, cl), "one tile pair per launch")
        assert st["launches"] == st["tiles_tested"]
    finally:
        L.cilhip_ccn_set_pair_cap(0)
    st = {}
    run(p, r2, form=1, stats=st)
    assert st["launches"] == 1


def test_cpp_mirrors_give_the_yardstick(tmp_path):
    import os
    import subprocess

    from test_components_refs_cpu import build_cpp

    here = os.path.dirname(os.path.abspath(__file__))
    exe = build_cpp(os.path.join(here, "cpp", "test_components_nd.cpp"), "test_components_nd")
    for dim, case in ((2, 1), (6, 5)):      # ConnectedComponentExtraction2f with a distance clause; Xf with distance + N-D normals
        p, r2 = R.evaluator_fixture(dim)[:2]
        name, args, cl = R.evaluator_cases(dim)[case]
        assert name == ("PointsProximityEvaluator", "PointsNormalsProximityEvaluator")[case == 5]
        fp, fn = str(tmp_path / f"p{dim}.f32"), "-"
        p.tofile(fp)
        if cl.normals is not None:
            fn = str(tmp_path / f"n{dim}.f32")
            cl.normals.tofile(fn)
        want = R.components(p, r2, cl)
        for form in (1, 2):
            pre = str(tmp_path / f"out{dim}_{form}")
            r = subprocess.run([exe, "run", str(dim), fp, fn, pre, repr(float(r2)), repr(float(cl.max_distance)), repr(float(cl.max_angle or 0.0)), str(form)], capture_output=True, text=True)
            assert r.returncode == 0 and "run OK" in r.stdout and f"form {form}" in r.stdout, r.stdout + r.stderr
            labels, members, sizes = (np.fromfile(pre + ext, np.uint64).astype(np.int64) for ext in (".labels.u64", ".members.u64", ".sizes.u64"))
            assert np.array_equal(labels, want[0]) and np.array_equal(sizes, np.diff(want[1])) and np.array_equal(members, want[2][:want[1][-1]])


def test_example_output():
    import os
    import subprocess

    from test_components_refs_cpu import build_cpp

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = build_cpp(os.path.join(root, "examples", "connected_component_extraction_nd.cpp"), "example_connected_component_extraction_nd")
    outs = []
    for _ in range(2):
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        outs.append([ln for ln in r.stdout.splitlines() if not ln.startswith("Segmentation time")])
    assert outs[0] == outs[1]      # C4
    text = "\n".join(outs[0])
    assert "Number of points: 1500 (dimension 6)" in text and "Form 1, sweep axis 0, tile pairs tested / total: 21 / 21, 1 launch(es)" in text      # form 0 at 1500 points: the triangle
    nseg = int(text.split("Number of segments: ")[1].split()[0])
    sizes = [int(v) for v in text.split("Segment sizes:")[1].splitlines()[0].replace("...", "").split()]
    assert nseg >= 3 and sizes == sorted(sizes, reverse=True) and sizes[2] > 100      # the three blobs, and what the clauses split off them
