"""The engine options of CorrespondenceSearchKDTree on the GPU -- inlier_fraction, one_to_one, the search directions FIRST_TO_SECOND
and BOTH, require_reciprocality (filters.hip, bidir.hip, the getter's order) -- element for element against what the reference
leaves, on fixtures whose distances are exact (tests/_filter_refs.py): few distinct values, so the radix select is decided in the
INDEX bytes of its keys; matches exactly on the (strict) radius; llround(f n) landing on halves; counts 0, 1 and around a wave and
a block; more entries than one trip of any kernel's grid; sources that several targets name and minima that several sources hold;
transforms that stay exact (a mirror, a scale, a singular matrix).

The expected lists are the restatement's over the fixtures' correspondence sets by construction; tests/test_filter_refs_cpu.py pins
both to the CPU oracle and shows that no fixture holds a nearest-neighbour tie in the searches run on it, so option tie_rule 2 (the
default) and 0 must agree: both run.  Every comparison is np.array_equal on the indices and on the distances' bits."""
import time

import numpy as np
import pytest

import _filter_refs as fr

pytestmark = pytest.mark.gpu

DIRS = (("second_to_first", fr.S2F, False), ("first_to_second", fr.F2S, False), ("both", fr.BOTH, False), ("both_reciprocal", fr.BOTH, True))
TIE_RULES = (2, 0)
_figures = {}


@pytest.fixture(scope="module")
def Context(hip_lib):
    from cilantro_amd.icp import Context as C

    return C


def _note(name, obj):
    """figures of the run: printed (pytest -s shows them) and kept for the assertions that read them"""
    _figures[name] = obj
    print(name, obj)


_full = {}


def _attached8():
    if "a" not in _full:
        _full["a"] = fr.attached(8, 1)
    return _full["a"]


def _context(Context, fix, transform="identity"):
    ctx = Context()
    ctx.set_target(fix["dst"]); ctx.set_source(fr.stored_source(fix["q"], transform))
    return ctx


def _search(ctx, T, fix, d, recip, f, o2o):
    ctx.set_option("search_direction", d); ctx.set_option("require_reciprocality", 1 if recip else 0)
    ctx.set_option("inlier_fraction", f); ctx.set_option("one_to_one", 1 if o2o else 0)
    n = ctx.find_correspondences(T, float(fix["max_sq"]))
    got = ctx.get_correspondences()
    assert n == len(got[0]), (fix["name"], d, recip, f, o2o, n, len(got[0]))
    return got


def _dirs_of(fix):
    return tuple(x for x in DIRS if (fix["fwd"] is not None or x[1] == fr.F2S) and (fix["rev"] is not None or x[1] == fr.S2F))


def _sweep(ctx, fix, T, fractions=None, search=_search):
    """every direction the fixture allows x every fraction x one-to-one off / on x both tie rules; -> lists compared, entries compared"""
    lists = entries = 0
    for rule in TIE_RULES:
        ctx.set_option("tie_rule", rule)
        for dname, d, recip in _dirs_of(fix):
            n = len(fr.expected(fix, d, recip)[0])
            for f in (list(fr.FRACTIONS) + fr.half_fractions(n)) if fractions is None else fractions:
                plain = search(ctx, T, fix, d, recip, f, False)
                exp = fr.expected(fix, d, recip, f, False)
                assert fr.same(plain, exp), (fix["name"], dname, rule, f, len(plain[0]), len(exp[0]))
                o2o = search(ctx, T, fix, d, recip, f, True)
                exp = fr.expected(fix, d, recip, f, True)
                assert fr.same(o2o, exp), (fix["name"], dname, rule, f, "one_to_one", len(o2o[0]), len(exp[0]))
                if d == fr.BOTH:
                    assert fr.same(o2o, plain), (fix["name"], dname, rule, f)      # correspondence.hpp:96-98: a no-op
                lists += 2; entries += len(plain[0]) + len(o2o[0])
    ctx.set_option("tie_rule", 2)
    return lists, entries


I4 = np.eye(4, dtype=np.float32)


@pytest.mark.parametrize("m", fr.COUNTS)
def test_every_option_at_a_match_count(Context, m):
    """the attached fixture cut to m forward matches: fractions that keep none, all, half, land on k + 1/2 (half away from zero) or do
    not filter (1.0, 0.0), in every direction, with and without one-to-one"""
    fix = fr.cut_matches(_attached8(), m)
    assert len(fix["fwd"][0]) == m
    for dname, d, recip in DIRS[:1] + DIRS[2:3]:
        n = len(fr.expected(fix, d, recip)[0])
        for f in fr.half_fractions(n) + ([0.5] if n % 2 else []):
            assert (f * n) % 1.0 == 0.5 and len(fr.expected(fix, d, recip, f)[0]) == int(f * n) + 1
    lists, entries = _sweep(_context(Context, fix), fix, I4)
    _note(f"count_{m}", {"targets": len(fix["dst"]), "sources": len(fix["q"]), "forward": m, "reverse": len(fix["rev"][0]), "lists": lists, "entries": entries})


def test_every_option_at_65537_sources(Context):
    fix = fr.cut_sources(fr.attached(28, 7), 65537)
    assert len(fix["q"]) == 65537
    lists, entries = _sweep(_context(Context, fix), fix, I4)
    _note("sources_65537", {"targets": len(fix["dst"]), "forward": len(fix["fwd"][0]), "reverse": len(fix["rev"][0]),
                            "distinct_values": len(np.unique(fr.bits(fix["fwd"][2]))), "lists": lists, "entries": entries})


def test_directions_and_filters_on_the_whole_fixtures(Context):
    """SECOND_TO_FIRST, FIRST_TO_SECOND, BOTH, BOTH + reciprocal, each with and without a fraction and one-to-one: the attached fixture
    (matches on the radius, 24 distinct values) and the shared one (BOTH's union holds pairs only the reverse search names)"""
    for fix in (_attached8(), fr.shared(8, 4)):
        both = fr.expected(fix, fr.BOTH, False); recip = fr.expected(fix, fr.BOTH, True)
        assert len(recip[0]) < len(both[0])
        lists, entries = _sweep(_context(Context, fix), fix, I4)
        _note(fix["name"], {"targets": len(fix["dst"]), "sources": len(fix["q"]), "forward": len(fix["fwd"][0]), "reverse": len(fix["rev"][0]),
                            "union": len(both[0]), "reciprocal": len(recip[0]), "on_radius": fix.get("on_radius"),
                            "distinct_values": len(np.unique(fr.bits(fix["fwd"][2]))), "lists": lists, "entries": entries})
    assert _figures["attached_8"]["on_radius"] > 0 and _figures["shared_8"]["union"] > _figures["shared_8"]["forward"]


def test_one_to_one_ties_go_to_the_lowest_index(Context):
    """tied_minima under SECOND_TO_FIRST (several sources at a target's smallest value: the lowest source index stays) and both shared
    fixtures under FIRST_TO_SECOND (two targets name one source, at 60 / 68 units and at 64 / 64: the lowest target index stays)"""
    ties = {}
    for fix, col in ((fr.attached(8, 3, tied=True), 0), (fr.shared(8, 4), 1), (fr.shared(8, 5, midpoint=True), 1)):
        t = fix["fwd"] if col == 0 else fix["rev"]
        named_twice, tied_at_min = fr.contended(t, col)
        ties[fix["name"]] = {"named_by_two_or_more": named_twice, "tied_at_the_smallest_value": tied_at_min}
        assert named_twice > 0
        if not fix["name"].startswith("shared_8"):
            assert tied_at_min > 0
        dirs = [x for x in _dirs_of(fix) if x[1] == (fr.S2F if col == 0 else fr.F2S)]
        assert len(dirs) == 1
        d = dirs[0][1]
        kept = fr.expected(fix, d, False, 1.0, True)
        assert len(kept[0]) == len(t[0]) - (np.bincount(t[col]).clip(1) - 1).sum() < len(t[0])
        ctx = _context(Context, fix)
        for rule in TIE_RULES:
            ctx.set_option("tie_rule", rule)
            n = len(t[0])
            for f in list(fr.FRACTIONS) + fr.half_fractions(n):
                for o2o in (False, True):
                    assert fr.same(_search(ctx, I4, fix, d, False, f, o2o), fr.expected(fix, d, False, f, o2o)), (fix["name"], rule, f, o2o)
    _note("ties", ties)


@pytest.mark.parametrize("name", list(fr.TRANSFORMS))
def test_exact_transforms(Context, name):
    """the source is stored as T^-1 of the fixture, exactly: the same lists under the identity, a quarter turn with an integer shift,
    a mirror (negative determinant), a uniform scale (smallest singular value 2) and the singular diag(1, 1, 0) (a planar lattice,
    sources with arbitrary z: find_pairs builds a grid over the transformed copy) -- through the engine class"""
    from cilantro_amd.icp import CorrespondenceSearchDirection as D, CorrespondenceSearchHIP

    T = fr.TRANSFORMS[name][0]
    fix = fr.attached(16, 2, planar=True) if name == "flatten_z" else _attached8()
    ctx = _context(Context, fix, name)
    eng = CorrespondenceSearchHIP(ctx=ctx).setMaxDistance(fix["max_sq"])
    code = {fr.S2F: D.SECOND_TO_FIRST, fr.F2S: D.FIRST_TO_SECOND, fr.BOTH: D.BOTH}

    def search(ctx_, T_, fix_, d, recip, f, o2o):
        eng.setSearchDirection(code[d]).setRequireReciprocality(recip).setInlierFraction(f).setOneToOne(o2o)
        return eng.findCorrespondences(T_).getCorrespondences()

    n = len(fix["fwd"][0])
    lists, entries = _sweep(ctx, fix, T, fractions=[0.5, 1.0] + fr.half_fractions(n)[:1], search=search)
    _note("transform_" + name, {"targets": len(fix["dst"]), "sources": len(fix["q"]), "forward": n, "reverse": len(fix["rev"][0]), "lists": lists, "entries": entries})


def test_past_one_trip_of_every_grid(Context):
    """262 144 targets, about 840 000 sources: more sources than filters.hip's 2048 x 256 lanes, more candidates under BOTH than bidir.hip's
    4096 x 256.  The expected lists come from the construction, through the restatement."""
    t0 = time.perf_counter()
    fix = fr.attached(64, 11)
    nd, ns = len(fix["dst"]), len(fix["q"])
    assert nd == 262144 and ns > 2048 * 256 and nd + ns > 4096 * 256
    t1 = time.perf_counter()
    ctx = _context(Context, fix)
    sizes = {}
    for dname, d, f, o2o in (("second_to_first", fr.S2F, 0.5, True), ("both", fr.BOTH, 0.5, False), ("first_to_second", fr.F2S, 1.0, True)):
        got = _search(ctx, I4, fix, d, False, f, o2o)
        exp = fr.expected(fix, d, False, f, o2o)
        assert fr.same(got, exp), (dname, len(got[0]), len(exp[0]))
        sizes[dname] = len(exp[0])
    assert len(fix["fwd"][0]) > 2048 * 256 and len(fix["fwd"][0]) > 2 * sizes["second_to_first"] and sizes["both"] > 2048 * 128
    _note("past_one_trip", {"targets": nd, "sources": ns, "forward": len(fix["fwd"][0]), "reverse": len(fix["rev"][0]), "kept": sizes,
                            "seconds_fixture": round(t1 - t0, 2), "seconds_rest": round(time.perf_counter() - t1, 2)})


def test_host_and_device_clouds(Context):
    """the same lists whether a cloud comes from host or from device memory"""
    import torch

    fix = _attached8()
    for dst_dev, src_dev in ((True, False), (False, True)):
        dst = torch.from_numpy(fix["dst"]).cuda() if dst_dev else fix["dst"]
        src = torch.from_numpy(fix["q"]).cuda() if src_dev else fix["q"]
        ctx = Context()
        ctx.set_target(dst); ctx.set_source(src)
        for dname, d, recip in DIRS:
            for o2o in (False, True):
                assert fr.same(_search(ctx, I4, fix, d, recip, 0.5, o2o), fr.expected(fix, d, recip, 0.5, o2o)), (dst_dev, src_dev, dname, o2o)
