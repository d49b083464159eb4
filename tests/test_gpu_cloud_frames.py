"""Search and ICP parity on clouds the other parity tests never build: rescaled by powers of two, moved away from the origin, and
source sizes at the loop's form switches.

Every other parity test runs either the synthetic recipe (points in [0, 1)^3) or the reference's sensor frames (within a metre of
the origin).  The exactness arguments of DESIGN.md 6 compare f32 geometry against bounds; what they leave to rounding scales with
|coordinate| (the cell faces the searches prune against are computed as `origin + c * cell` in absolute f32) or with the cloud's
size (the kernels deal the source out in fixed rounds, tiles and partial rows).  Here:
  * 2^k rescaling is a metamorphic test, exact by construction: a power of two commutes with every pinned f32 expression and with
    the f64 solve as long as nothing under- or overflows, so matches, d2 bits and the transform must follow exactly;
  * clouds at offsets up to 16384 (coordinates quantised far more coarsely than the point spacing: exact ties), a 1 cm object at
    100, a cloud straddling zero: every search form, the loop's own matches, the reverse directions, kNN lists and KMeans labels
    against the reference's nanoflann (or the oracle kd-tree) and the oracle loop;
  * source sizes at 65535 / 65536 / 65537 (the warm-started form's floor), off a multiple of 64 / 256 / 2048, 1-3 points, a
    target of 1-8 points, and the accumulated sums at sizes that leave partial waves.
Measured counts are written as cloud_frames_*.json by _report (test_gpu_loop_matches.py), next to the other reports.
"""
import numpy as np
import pytest

from cilantro_amd import capi
from cilantro_amd import synthetic as syn
from test_gpu_loop_matches import _check_against_fresh_search_and_reference, _classify, _params, _report, _signed
from test_gpu_parity import _oracle_icp_loop

pytestmark = pytest.mark.gpu

WARM_FORMS = (2, 3)         # cilhip_get_last_form_timing codes: 0 search alone, 1 tiled one pass, 2/3 warm-started, 4 fused per-lane


@pytest.fixture(scope="module")
def Context(hip_lib):
    from cilantro_amd.icp import Context as Ctx

    return Ctx


@pytest.fixture(scope="module")
def base_1m():
    return syn.make_pair(1_000_000)


def _moved(d, scale=1.0, offset=0.0):
    """the recipe's pair scaled and moved in f64, rounded once to f32 (the motion between the clouds is unchanged in the cloud's own
    frame, so a loop from the identity has the same work to do; its transform's translation grows with the offset)"""
    off = np.broadcast_to(np.asarray(offset, np.float64), (3,))
    f = lambda a: np.ascontiguousarray((a.astype(np.float64) * scale + off).astype(np.float32))
    return {"dst": f(d["dst"]), "dst_n": d["dst_n"], "src": f(d["src"]), "max_sq_dist": np.float32(float(d["max_sq_dist"]) * scale * scale)}


def _has_duplicates(P):
    return len(np.unique(P.view(np.dtype((np.void, 12))))) < len(P)


def _run_loop(Context, D, N, S, r2, iters, options=(), metric=capi.METRIC_COMBINED, conv_tol=0.0):
    ctx = Context()
    for k, v in options:
        ctx.set_option(k, v)
    ctx.set_target(D, N)
    ctx.set_source(S)
    p = _params(ctx, metric, 0.0, r2, iters)
    p.conv_tol = conv_tol
    res = ctx.icp_run(p)
    out = {"T": np.array(res.T[:], np.float32).reshape(4, 4).T.copy(), "iterations": int(res.iterations), "ncorr": int(res.last_ncorr),
           "trace": [t["form"] for t in ctx.last_run_trace()], "warm": ctx.last_warm_iterations(), "origin": ctx.last_matches_origin(),
           "Tm": ctx.matches_transform()}
    idx, d2 = ctx.get_nn()
    out["idx"], out["d2"] = _signed(idx), d2.copy()
    ctx.close()
    return out


def _search(Context, D, N, S, T, r2, options=()):
    ctx = Context()
    for k, v in options:
        ctx.set_option(k, v)
    ctx.set_target(D, N)
    ctx.set_source(S)
    ctx.find_correspondences(T, float(r2), count=False)
    assert ctx.last_matches_origin() == 3
    if dict(options).get("search_direction", 0):
        pairs = ctx.get_correspondences()
        ctx.close()
        return None, None, pairs
    idx, d2 = ctx.get_nn()
    ctx.close()
    return _signed(idx), d2.copy(), None


# --------------------------------------------------------------------------------------------------------------------------------
# 1. power-of-two rescaling: exact by construction
# --------------------------------------------------------------------------------------------------------------------------------

SEARCH_FORMS = (("per lane", (("tiled", 0), ("group_search", 0))), ("tiles", (("tiled", 2),)), ("8 lanes per query", (("tiled", 0), ("group_search", 8))))
LOOP_FORMS = (("default", (), capi.METRIC_COMBINED), ("warm forced", (("warm_start", 2),), capi.METRIC_COMBINED),
              ("tiles one pass", (("warm_start", 0), ("tiled", 2), ("tile_accumulation", 2)), capi.METRIC_COMBINED),
              ("fused per lane", (("fused", 1),), capi.METRIC_COMBINED), ("point-to-point", (), capi.METRIC_POINT_TO_POINT))


def test_power_of_two_rescaling_is_exact(Context, orc, base_1m):
    """x -> 2^k x (coordinates, translation, sqrt(r2)): every search form names the same points with d2 * 4^k bit for bit (nearest
    neighbours, FIRST_TO_SECOND / BOTH pairs, kNN lists, radius lists); every loop form runs the same kernel forms iteration by
    iteration, leaves the same matches, the same rotation block bit for bit and 2^k times the translation bit for bit.  An absolute
    constant hiding in a margin, an entry test or a bound would show as another form or another match at some scale."""
    from cilantro_amd.normal_estimation import KDTree3f

    rng = np.random.default_rng(41)
    T0 = base_1m["T_true"].astype(np.float32)
    qs = rng.choice(len(base_1m["src"]), 20_000, replace=False)
    ref = {}
    report = {}
    bad = []
    for k in (0, -24, -12, 12, 24):
        s = 2.0 ** k
        d = _moved(base_1m, scale=s)
        D, N, S, r2 = d["dst"], d["dst_n"], d["src"], d["max_sq_dist"]
        s4 = np.float32(4.0 ** k)
        T = T0.copy()
        T[:3, 3] *= np.float32(s)
        got = {}
        for fname, opts in SEARCH_FORMS:
            gi, gd, _ = _search(Context, D, N, S, T, r2, opts)
            got[("nn", fname)] = (gi, gd)
        for dname, code in (("FIRST_TO_SECOND", 1), ("BOTH", 2)):
            _, _, (i1, i2, v) = _search(Context, D, N, S, T, r2, (("search_direction", code),))
            got[("pairs", dname)] = (np.stack([i1, i2]), v)
        tree = KDTree3f(D)
        qk = orc.transform_points(T, S[qs])
        ki, kd, kc = tree.kNNSearch(qk, 8)
        got[("knn", 8)] = (ki, kd)
        off, ri, rd = tree.radiusSearch(qk[:2000], r2)
        got[("radius", 0)] = (np.concatenate([off, ri]), rd)
        for fname, opts, metric in LOOP_FORMS:
            r = _run_loop(Context, D, N, S, r2, 8, opts, metric)
            got[("loop", fname)] = r
            if fname == "default":
                report[f"2^{k}/default/vs reference"] = _check_against_fresh_search_and_reference(
                    Context, orc, (k, fname), D, N, S, r2, r["idx"], r["d2"], r["Tm"], r["ncorr"], 50_000, rng, False)
        if k == 0:
            ref = got
            # the forms the options name really ran (and, below, the same ones at every scale)
            for fname, opts, metric in LOOP_FORMS:
                r = got[("loop", fname)]
                report[f"forms/{fname}"] = {"trace": r["trace"], "origin": r["origin"], "warm": r["warm"]}
                if fname in ("default", "warm forced") and r["warm"] == 0:
                    bad.append((k, fname, "no warm-started iteration", r["trace"]))
                if fname == "warm forced" and not (r["warm"] == 7 and all(f in WARM_FORMS for f in r["trace"][1:])):
                    bad.append((k, fname, "form", r["trace"]))
                if fname == "tiles one pass" and not (r["origin"] == 2 and set(r["trace"]) == {1}):
                    bad.append((k, fname, "form", r["origin"], r["trace"]))
                if fname == "fused per lane" and not (r["origin"] == 2 and set(r["trace"]) == {4}):
                    bad.append((k, fname, "form", r["origin"], r["trace"]))
            continue
        for key, val in got.items():
            if key[0] == "loop":
                a, b = val, ref[key]
                if a["trace"] != b["trace"] or a["warm"] != b["warm"] or a["iterations"] != b["iterations"]:
                    bad.append((k, key, "kernel forms", a["trace"], b["trace"]))
                if a["ncorr"] != b["ncorr"] or not np.array_equal(a["idx"], b["idx"]):
                    bad.append((k, key, "matches", int(np.count_nonzero(a["idx"] != b["idx"]))))
                    continue
                m = a["idx"] >= 0
                if not np.array_equal(a["d2"][m].view(np.uint32), (b["d2"][m] * s4).view(np.uint32)):
                    bad.append((k, key, "d2 bits"))
                rot_exact = np.array_equal(a["T"][:3, :3].view(np.uint32), b["T"][:3, :3].view(np.uint32))
                tr_exact = np.array_equal(a["T"][:3, 3].view(np.uint32), (b["T"][:3, 3] * np.float32(s)).view(np.uint32))
                if not (rot_exact and tr_exact):
                    # (the step named here is not exactly equivariant: the transform within 1e-6 relative, recorded)
                    rot = float(np.abs(a["T"][:3, :3].astype(np.float64) - b["T"][:3, :3]).max())
                    tr = float(np.abs(a["T"][:3, 3].astype(np.float64) / s - b["T"][:3, 3]).max() / max(np.abs(b["T"][:3, 3]).max(), 1e-30))
                    report[f"2^{k}/{key[1]}/transform not bitwise"] = {"rotation": rot, "translation_rel": tr}
                    if rot > 1e-6 or tr > 1e-6:
                        bad.append((k, key, "transform", rot, tr))
                continue
            (ai, ad), (bi, bd) = val, ref[key]
            if not np.array_equal(ai, bi):
                bad.append((k, key, "indices", int(np.count_nonzero(ai != bi))))
                continue
            m = np.isfinite(bd) if key[0] == "knn" else (bi >= 0 if key[0] == "nn" else np.ones(len(bd), bool))
            if not np.array_equal(ad[m].view(np.uint32), (bd[m] * s4).view(np.uint32)):
                bad.append((k, key, "d2 bits"))
    report["failures"] = [str(b) for b in bad]
    _report("cloud_frames_rescaled.json", report)
    assert not bad, bad


# --------------------------------------------------------------------------------------------------------------------------------
# 2. clouds away from the origin
# --------------------------------------------------------------------------------------------------------------------------------

def _offset_clouds(base_1m):
    small = syn.make_pair(200_000)
    mid = syn.make_pair(500_000)
    return (("unit cube at (1e3, -250, 37)", _moved(base_1m, offset=(1e3, -250.0, 37.0))),
            ("unit cube at 4096", _moved(base_1m, offset=4096.0)),
            ("unit cube at 16384", _moved(base_1m, offset=16384.0)),
            ("1 cm object at 100", _moved(small, scale=0.01, offset=100.0)),
            ("extent 1e3 across zero", _moved(mid, scale=1e3, offset=-500.0)))


@pytest.mark.parametrize("which", range(5))
def test_clouds_away_from_the_origin(Context, orc, base_1m, which):
    """Every search form, the loop's own matches in the per-lane / one-pass tile / warm-started forms, the reverse directions
    (warm-started reverse searches), kNN lists and KMeans labels on a cloud far from the origin, index for index against the
    reference's nanoflann (or the oracle kd-tree) and the oracle.  The transforms: the rotation block within 1e-5 of the oracle
    loop's (MODE_MIXED), the translation within 1e-5 * (1 + max |centroid|) -- its entries are of the order of the rotation's
    angle times the offset and carry the rounding of f32 values of that magnitude, so an absolute 1e-5 is not reachable there.
    At 16384 the per-lane form (the oracle's order of the f64 additions) still equals the oracle bit for bit, but a form that adds
    in another order may end one ulp of T away after some iteration, and there one ulp of the rotation moves a query by about its
    own ulp (2^-9): other matches, other sums -- a different, equally exact trajectory (its matches are checked at its own transform
    like every other's).  Those forms' transforms are held to 1e-3 there (measured: 1.6e-4 / 3.2e-4 rotation) and recorded."""
    from cilantro_amd.clustering import kmeans_assign
    from cilantro_amd.normal_estimation import KDTree3f

    name, d = _offset_clouds(base_1m)[which]
    rng = np.random.default_rng(50 + which)
    D, N, S, r2 = d["dst"], d["dst_n"], d["src"], d["max_sq_dist"]
    ties = _has_duplicates(D)
    tree = orc.KDTree(D, use_ref=orc.ref_available())
    po = orc.make_params(metric=1, max_iter=6, conv_tol=0.0, max_sq_dist=float(r2), mode=orc.MODE_MIXED)
    To, nco = _oracle_icp_loop(orc, tree, d, po, 6)
    cmax = float(np.abs(D.astype(np.float64).mean(axis=0)).max())
    report = {"cloud": name, "points": int(len(D)), "duplicate target positions": bool(ties), "oracle last_ncorr": int(nco)}
    failures = []

    # search-only forms under the oracle's final transform
    sample = np.sort(rng.choice(len(S), min(50_000, len(S)), replace=False))
    o1, o2, ov = tree.find_correspondences(orc.transform_points(To, S[sample]), float(r2))
    oi = np.full(len(sample), -1, np.int64); od = np.zeros(len(sample), np.float32)
    oi[o2] = o1; od[o2] = ov
    first = None
    for fname, opts in (("per lane", (("tiled", 0), ("group_search", 0))), ("tiles", (("tiled", 2),)),
                        ("8 lanes per query", (("tiled", 0), ("group_search", 8))), ("16 lanes per query", (("tiled", 0), ("group_search", 16)))):
        gi, gd, _ = _search(Context, D, N, S, To, r2, opts)
        nbad, nt, nn, nw = _classify(gi[sample], gd[sample], oi, od)
        report[f"search/{fname}"] = {"mismatches": nbad, "ties": nt, "nearer": nn, "worse": nw}
        if nn or nw or (nbad and not ties):
            failures.append(("search", fname, nbad, nt, nn, nw))
        if first is None:
            first = (gi, gd)
        elif not np.array_equal(gi, first[0]) or not np.array_equal(gd[gi >= 0].view(np.uint32), first[1][gi >= 0].view(np.uint32)):
            failures.append(("search forms disagree", fname, int(np.count_nonzero(gi != first[0]))))

    # the loop's own matches after 6 iterations
    for fname, opts, origin, forms in (("per lane, cold", (("warm_start", 0), ("tiled", 0), ("group_search", 0)), 1, {0}),
                                       ("tiles one pass", (("warm_start", 0), ("tiled", 2), ("tile_accumulation", 2)), 2, {1}),
                                       ("warm forced", (("warm_start", 2), ("tiled", 2)), 1, None)):
        r = _run_loop(Context, D, N, S, r2, 6, opts)
        ran = set(r["trace"]) == forms if forms is not None else (r["warm"] == 5 and all(f in WARM_FORMS for f in r["trace"][1:]))
        if r["iterations"] != 6 or r["origin"] != origin or not ran:
            failures.append(("loop form", fname, r["iterations"], r["origin"], r["trace"]))
        try:
            chk = _check_against_fresh_search_and_reference(Context, orc, (name, fname), D, N, S, r2, r["idx"], r["d2"], r["Tm"], r["ncorr"],
                                                            50_000, rng, ties, tree=tree)
        except AssertionError as e:
            chk = {"failed": str(e)[:400]}
            failures.append(("loop matches", fname, str(e)[:200]))
        rot = float(np.abs(r["T"][:3, :3].astype(np.float64) - To[:3, :3]).max())
        tr = float(np.abs(r["T"][:3, 3].astype(np.float64) - To[:3, 3]).max())
        chk.update({"forms": r["trace"], "rotation_vs_oracle": rot, "translation_vs_oracle": tr, "ncorr": r["ncorr"]})
        report[f"loop/{fname}"] = chk
        tol = 1e-3 if (cmax >= 16384.0 and fname != "per lane, cold") else 1e-5
        if rot > tol or tr > tol * (1.0 + cmax) or r["ncorr"] != nco:
            failures.append(("loop transform", fname, rot, tr, r["ncorr"], nco))

    # reverse directions, warm-started reverse searches: the last pair list against the oracle's at the transform it was found under
    for dname, code in (("FIRST_TO_SECOND", 1), ("BOTH", 2)):
        ctx = Context()
        ctx.set_option("search_direction", code); ctx.set_option("reverse_warm_start", 1)
        ctx.set_target(D, N); ctx.set_source(S)
        ctx.icp_run(_params(ctx, capi.METRIC_COMBINED, 0.0, r2, 6))
        assert ctx.get_option("reverse_warm_start") == 1
        Tm = ctx.matches_transform()
        g1, g2, gv = ctx.get_correspondences()
        ctx.close()
        e1, e2, ev = orc.find_correspondences_dir(D, orc.transform_points(Tm, S), float(r2), code)
        same = len(g1) == len(e1) and np.array_equal(g1, e1) and np.array_equal(g2, e2) and np.array_equal(gv.view(np.uint32), ev.view(np.uint32))
        report[f"reverse/{dname}"] = {"pairs": int(len(g1)), "oracle pairs": int(len(e1)), "identical": bool(same)}
        if not same:
            failures.append(("reverse", dname, len(g1), len(e1)))

    # kNN lists (k = 8) at the source's points under the oracle's transform
    q = orc.transform_points(To, S[sample[:20_000]])
    gi, gd, gc = KDTree3f(D).kNNSearch(q, 8)
    if tree.use_ref:
        ki, kd, kc = orc.ref_knn_batch(tree, q, 8, num_threads=16)
    else:
        ki, kd, kc = orc.knn_batch(tree, q, 8)
    knn_rows = int(np.count_nonzero((gi != ki).any(axis=1) | (gd != kd).any(axis=1)))
    report["knn8 rows differing"] = knn_rows
    if knn_rows:
        failures.append(("knn", knn_rows))

    # KMeans labels, brute-force grid branch and kd-tree branch
    x = D[rng.choice(len(D), min(200_000, len(D)), replace=False)]
    cent = np.ascontiguousarray(x[:: len(x) // 64][:64])
    for kd_tree in (False, True):
        lg = kmeans_assign(x, cent, use_kd_tree=kd_tree)
        lo, _ = orc.kmeans_assign(x, cent, use_kd_tree=kd_tree)
        nlab = int(np.count_nonzero(lg != lo))
        report[f"kmeans labels differing (kd tree {kd_tree})"] = nlab
        if nlab:
            failures.append(("kmeans", kd_tree, nlab))
    report["failures"] = [str(f) for f in failures]
    _report(f"cloud_frames_offset_{which}.json", report)
    assert not failures, (name, failures)


# --------------------------------------------------------------------------------------------------------------------------------
# 3. sizes at the loop's form switches
# --------------------------------------------------------------------------------------------------------------------------------

def _vs_oracle_loop(Context, orc, D, N, S, r2, iters, options, metric, name, tree):
    r = _run_loop(Context, D, N, S, r2, iters, options, metric)
    po = orc.make_params(metric=metric, max_iter=iters, conv_tol=0.0, max_sq_dist=float(r2), mode=orc.MODE_MIXED)
    ro = orc.icp_run(D, N if metric == 1 else None, S, po)
    err = float(np.linalg.norm(r["T"].astype(np.float64) - ro["T"].astype(np.float64)))
    if len(S) <= 2 and metric == 0:
        # two correspondences leave the rotation about the line through them free: the SVD's choice is not part of the contract,
        # where the transforms put the source points is
        err = float(np.abs(orc.transform_points(r["T"], S).astype(np.float64) - orc.transform_points(ro["T"], S)).max())
    assert r["iterations"] == ro["iterations"], (name, r["iterations"], ro["iterations"])
    if metric == 0 or len(S) >= 6:
        assert err <= 1e-5 and r["ncorr"] == ro["last_ncorr"], (name, err, r["ncorr"], ro["last_ncorr"])
    # (point-to-plane with fewer than 6 correspondences: 6 unknowns, rank-deficient normal equations -- the step is whatever the
    #  rounding leaves in the last pivots, on either side; only the loop's own matches below are defined)
    # the last iteration's matches: the kd-tree's at the transform they were found under
    assert r["origin"] in (1, 2), (name, r["origin"])
    o1, o2, ov = tree.find_correspondences(orc.transform_points(r["Tm"], S), float(r2))
    oi = np.full(len(S), -1, np.int64); od = np.zeros(len(S), np.float32)
    oi[o2] = o1; od[o2] = ov
    assert np.array_equal(r["idx"], oi), (name, np.nonzero(r["idx"] != oi)[0][:10])
    m = oi >= 0
    assert np.array_equal(r["d2"][m].view(np.uint32), od[m].view(np.uint32)), name
    return r, ro


def test_warm_start_floor_sizes(Context, orc):
    """ns = 65535 / 65536 / 65537 / 65536 + 255 / 65536 + 257 (the warm-started form's floor, rounds of 256 queries, one query past a
    round): the loop against the oracle's -- transform, last_ncorr, iteration count, the last matches index for index -- with the
    default options and with warm_start = 2; warm-started iterations ran exactly when ns >= 65536."""
    base = syn.make_pair(200_000, 65_793)
    tree = orc.KDTree(base["dst"], use_ref=orc.ref_available())
    report = {}
    for ns in (65535, 65536, 65537, 65536 + 255, 65536 + 257):
        S = np.ascontiguousarray(base["src"][:ns])
        for oname, opts in (("default", ()), ("warm forced", (("warm_start", 2),))):
            r, _ = _vs_oracle_loop(Context, orc, base["dst"], base["dst_n"], S, base["max_sq_dist"], 8, opts, 1, (ns, oname), tree)
            report[f"{ns}/{oname}"] = {"warm": r["warm"], "forms": r["trace"]}
            if ns < 65536:
                assert r["warm"] == 0 and not set(r["trace"]) & set(WARM_FORMS), (ns, oname, r["trace"])
            elif oname == "warm forced":
                assert r["warm"] == 7 and all(f in WARM_FORMS for f in r["trace"][1:]), (ns, r["trace"])
    _report("cloud_frames_floor_sizes.json", report)


def test_small_and_odd_source_sizes(Context, orc):
    """ns = 1, 2, 3, 5, 63, 65, 2047, 2049 (1-2 correspondences are degenerate in the reference: the loop follows the oracle's
    ok / identity result), per-lane and tiled, separate and fused, point-to-plane and point-to-point, against the oracle loop."""
    base = syn.make_pair(20_000)
    tree = orc.KDTree(base["dst"], use_ref=orc.ref_available())
    for ns in (1, 2, 3, 5, 63, 65, 2047, 2049):
        S = np.ascontiguousarray(base["src"][:ns])
        for tiled in (0, 2):
            for fused in (0, 1):
                for metric in (1, 0):
                    opts = (("tiled", tiled), ("fused", fused))
                    r, _ = _vs_oracle_loop(Context, orc, base["dst"], base["dst_n"], S, base["max_sq_dist"], 6, opts, metric, (ns, tiled, fused, metric), tree)
                    if fused:
                        assert set(r["trace"]) <= {4}, (ns, tiled, metric, r["trace"])
                    else:
                        assert 4 not in r["trace"] and r["warm"] == 0, (ns, tiled, metric, r["trace"])


def test_tiny_targets_against_brute_force(Context, orc):
    """a target of 1, 2 and 8 points against a 100k-point source: every search form against the exhaustive argmin"""
    rng = np.random.default_rng(61)
    S = rng.random((100_000, 3), dtype=np.float32)
    for nd in (1, 2, 8):
        D = rng.random((nd, 3), dtype=np.float32)
        for r2 in (np.float32(0.05), np.float32(3.4e38)):
            bi, bd = orc.nn_brute(D, S, float(r2))
            for opts in ((("tiled", 0), ("group_search", 0)), (("tiled", 2),), (("tiled", 0), ("group_search", 8))):
                gi, gd, _ = _search(Context, D, None, S, np.eye(4, dtype=np.float32), r2, opts)
                assert np.array_equal(gi, bi), (nd, r2, opts, np.nonzero(gi != bi)[0][:10])
                m = bi >= 0
                assert np.array_equal(gd[m].view(np.uint32), bd[m].view(np.uint32)), (nd, r2, opts)


def test_accumulated_sums_at_partial_wave_sizes(Context, orc):
    """estimate_point_to_point / estimate_combined over ns = 63, 65, 65537 correspondences (a partial wave, one past a wave, one
    past the warm floor): the sums against the oracle at 1e-9 relative -- tail lanes that add garbage instead of zeros show here"""
    base = syn.make_pair(200_000, 65_537)
    T = syn.true_transform(base["h"], 0.1).astype(np.float32)
    for ns in (63, 65, 65537):
        S = np.ascontiguousarray(base["src"][:ns])
        ctx = Context()
        ctx.set_target(base["dst"], base["dst_n"]); ctx.set_source(S)
        ctx.find_correspondences(T, base["max_sq_dist"])
        g1, g2, _ = ctx.get_correspondences()
        assert len(g1) > 0.9 * ns
        q = orc.transform_points(T, S)
        dm, sm = ctx.means()
        smt = orc.transform_points(T, sm.reshape(1, 3))[0]
        Tg, sums_g, ok = ctx.estimate_point_to_point()
        To, sums_o, ok2 = orc.estimate_p2p(base["dst"], q, g1, g2, orc.MODE_MIXED)
        assert ok == ok2
        np.testing.assert_allclose(sums_g, sums_o, rtol=1e-9, atol=1e-9 * np.abs(sums_o).max())
        for w_p2p, w_p2pl in ((0.0, 1.0), (1.0, 0.0), (0.1, 1.0)):
            Tg, AtA, Atb, cv = ctx.estimate_combined(w_p2p, w_p2pl, 1, 1e-5)
            To, AtAo, Atbo, cvo = orc.estimate_combined(base["dst"], base["dst_n"], q, g1, g2, w_p2p, w_p2pl, dm, smt, 1, 1e-5, orc.MODE_MIXED)
            scale = np.abs(AtAo).max()
            # (each term is formed in f32 as the reference forms it; over 63 terms those roundings, 2^-22 of a term, no longer average
            #  out below 1e-9 of the sum -- a tail lane that adds anything adds a whole term, ~1/ns of it)
            tol = 1e-9 * scale + (2.0 ** -22) * scale * (ns < 1000)
            assert np.abs(AtA - AtAo).max() <= tol, (ns, w_p2p, w_p2pl, np.abs(AtA - AtAo).max() / scale)
            assert np.abs(Atb - Atbo).max() <= 1e-9 * max(np.abs(Atbo).max(), 1e-30) + 1e-12 * scale + (tol - 1e-9 * scale), (ns, w_p2p, w_p2pl)
            assert np.linalg.norm(Tg.astype(np.float64) - To) < 1e-6 and cv == cvo, (ns, w_p2p, w_p2pl)
        ctx.close()
