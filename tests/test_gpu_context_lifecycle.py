"""GPU: the lifetimes of a context's device buffers (csrc/device_mem.hpp owns every allocation).  One long-lived context driven
through a fixed script of targets, sources and options gives, after every search and run, what a FRESH context configured the
same way gives -- correspondence lists element for element, transforms bit for bit; a target shared along a chain of three
contexts survives every order of closing them; and after every context is closed, and around each stateless entry point,
cilhip_debug_live_allocations reads the count and the bytes it read before: nothing is left behind, nothing is freed twice.
Sizes: 70 000 source points (above the 65 536 floor of the warm-started form: its buffers exist), option tiled = 2 (the tile
arrays exist), 3 500 target points doubled (every search of them ties: the order tables get built)."""
import ctypes as C

import numpy as np
import pytest

from cilantro_amd import capi, synthetic as syn

pytestmark = pytest.mark.gpu

NS, ND = 70_000, 3_500


def live(L):
    out = (C.c_ulonglong * 2)()
    assert L.cilhip_debug_live_allocations(out) == capi.OK
    return int(out[0]), int(out[1])


def doubled(d):
    return np.ascontiguousarray(np.concatenate([d["dst"], d["dst"]])), np.ascontiguousarray(np.concatenate([d["dst_n"], d["dst_n"]]))


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(5)
    a = syn.make_pair(ND, NS, perturb=0.3)
    b = syn.make_pair(5_000, NS, perturb=0.3)
    DA, NA = doubled(a)
    return {"A": (DA, NA), "B": (b["dst"], b["dst_n"]), "src": a["src"], "src_n": syn.make_normals(NS, seed=47),
            "rgb_A": rng.random((len(DA), 3), dtype=np.float32), "rgb_src": rng.random((NS, 3), dtype=np.float32),
            "r2": float(a["max_sq_dist"]), "T": syn.true_transform(a["h"], 0.2).astype(np.float32)}


def params(L, r2, iters):
    p = capi.IcpParams()
    L.cilhip_icp_default_params(C.byref(p))
    p.metric, p.w_p2p, p.w_p2pl = capi.METRIC_COMBINED, 0.1, 1.0
    p.max_sq_dist, p.max_iter, p.conv_tol = r2, iters, 0.0
    return p


class Model:
    """what the long-lived context has been told, in the order a fresh one is told it"""

    def __init__(self, cl):
        self.cl, self.opts = cl, {"tiled": 2}
        self.target = self.src = self.src_n = self.rgb = None

    def configure(self, c):
        for k, v in self.opts.items():
            c.set_option(k, v)
        c.set_target(*self.target)
        c.set_source(self.src, self.src_n)
        if self.rgb is not None:
            c.set_color_features(*self.rgb)
        return c


def same_search(live_ctx, m, T, r2):
    from cilantro_amd.icp import Context

    live_ctx.find_correspondences(T, r2)
    a = live_ctx.get_correspondences()
    f = m.configure(Context())
    f.find_correspondences(T, r2)
    b = f.get_correspondences()
    f.close()
    assert len(a[0]) == len(b[0]) and len(a[0]) > 0
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32))


def same_run(live_ctx, m, p):
    from cilantro_amd.icp import Context

    out = []
    f = m.configure(Context())
    for c in (live_ctx, f):
        r = c.icp_run(p)
        out.append((np.array(r.T[:], np.float32), int(r.iterations), int(r.last_ncorr), c.get_correspondences()))
    f.close()
    (Ta, ia, na, ca), (Tb, ib, nb, cb) = out
    assert np.array_equal(Ta.view(np.uint32), Tb.view(np.uint32)) and ia == ib and na == nb and na > 0
    assert len(ca[0]) == len(cb[0]) and all(np.array_equal(x, y) for x, y in zip(ca[:2], cb[:2]))
    assert np.array_equal(ca[2].view(np.uint32), cb[2].view(np.uint32))
    return Ta


def test_long_lived_context_matches_fresh_ones(hip_lib, clouds):
    from cilantro_amd.icp import Context

    L, cl = capi.load(), clouds
    before = live(L)
    m, c = Model(cl), Context()
    r2, T = cl["r2"], cl["T"]
    half = np.ascontiguousarray(cl["src"][: NS // 2])

    def opt(k, v):
        c.set_option(k, v); m.opts[k] = v

    # 1. target A, source, a combined-metric run
    opt("tiled", 2)
    m.target, m.src = cl["A"], cl["src"]
    c.set_target(*m.target); c.set_source(m.src)
    first = same_run(c, m, params(L, r2, 6))
    assert c.tie_order_info()["loaded"]                                        # (the doubled points tied: the order tables exist)
    # 2. a smaller source, 3. a larger one
    for s in (half, cl["src"]):
        m.src = s
        c.set_source(s)
        same_run(c, m, params(L, r2, 6))
    # 4. source normals on (the symmetric objective streams them), then off
    m.src_n = cl["src_n"]
    c._ck(L.cilhip_set_source_normals(c._h, m.src_n.ctypes.data, capi.MEM_HOST))
    same_run(c, m, params(L, r2, 6))
    m.src_n = None
    c._ck(L.cilhip_set_source_normals(c._h, None, capi.MEM_HOST))
    same_run(c, m, params(L, r2, 6))
    # 5. 9-D point + normal + colour features (they need the source's normals again)
    m.src_n, m.rgb = cl["src_n"], (cl["rgb_A"], cl["rgb_src"])
    c._ck(L.cilhip_set_source_normals(c._h, m.src_n.ctypes.data, capi.MEM_HOST))
    c.set_color_features(*m.rgb)
    opt("feature_kind", 2); opt("feature_normal_weight", 0.05); opt("feature_color_weight", 0.05)
    same_search(c, m, T, r2)
    # 6. BOTH directions, reciprocal: the source's grid, the pair list and the reverse buffers exist
    opt("feature_kind", 0); opt("feature_normal_weight", 0.0); opt("feature_color_weight", 0.0)
    opt("search_direction", 2); opt("require_reciprocality", 1)
    same_search(c, m, T, r2)
    same_run(c, m, params(L, r2, 4))
    # 7. the post-filters
    opt("search_direction", 0); opt("require_reciprocality", 0); opt("one_to_one", 1); opt("inlier_fraction", 0.7)
    same_search(c, m, T, r2)
    # 8. a target of another size: everything that described A goes (its colours too)
    opt("one_to_one", 0); opt("inlier_fraction", 1.0)
    m.target, m.rgb, m.src_n = cl["B"], None, None
    c.set_target(*m.target)
    c._ck(L.cilhip_set_source_normals(c._h, None, capi.MEM_HOST))
    same_search(c, m, T, r2)
    same_run(c, m, params(L, r2, 6))
    # 9. the first run again
    m.target = cl["A"]
    c.set_target(*m.target)
    again = same_run(c, m, params(L, r2, 6))
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32))
    c.close()
    assert live(L) == before


def test_shared_target_survives_every_closing_order(hip_lib, clouds):
    from cilantro_amd.icp import Context

    L, cl = capi.load(), clouds
    before = live(L)
    p = params(L, cl["r2"], 4)

    def run(ctx):
        r = ctx.icp_run(p)
        idx, d2 = ctx.get_nn()
        return bytes(np.array(r.T[:], np.float32)), int(r.last_ncorr), idx.tobytes(), d2[idx != capi.NONE_IDX].tobytes()

    def built(target):
        ctx = Context(); ctx.set_option("tiled", 2); ctx.set_target(*target); ctx.set_source(cl["src"])
        return ctx

    own = {}
    for name in ("A", "B"):
        ctx = built(cl[name]); own[name] = run(ctx); ctx.close()

    def chain():
        a = built(cl["A"])
        assert run(a) == own["A"]                                             # (what it has built by now -- the order tables -- is lent too)
        b, c = Context(), Context()
        for ctx, lender in ((b, a), (c, b)):                                     # a borrower lends on
            ctx.set_option("tiled", 2); ctx.share_target(lender); ctx.set_source(cl["src"])
            assert ctx.grid_info().build_ms == 0.0 and ctx.tie_order_info()["loaded"] and ctx.tie_order_info()["builds"] == 0
        return {"a": a, "b": b, "c": c}

    for order in ("abc", "cba", "bac"):
        ctxs = chain()
        for name in order:
            ctxs.pop(name).close()
            for survivor in ctxs.values():
                assert run(survivor) == own["A"]
    # the middle holder is given another target while the others live
    ctxs = chain()
    ctxs["b"].set_target(*cl["B"])
    assert run(ctxs["b"]) == own["B"] and run(ctxs["a"]) == own["A"] and run(ctxs["c"]) == own["A"]
    ctxs.pop("a").close()
    assert run(ctxs["c"]) == own["A"] and run(ctxs["b"]) == own["B"]
    for ctx in ctxs.values():
        ctx.close()
    assert live(L) == before


def test_stateless_calls_leave_nothing_behind(hip_lib):
    from cilantro_amd import clustering, grid_downsampler, model_estimation as me, normal_estimation as ne

    L = capi.load()
    n = 20_000
    d = syn.make_pair(n, perturb=0.2)
    P, h = d["dst"], d["h"]
    far = P.copy()
    far[0], far[1] = 3.0e38, -3.0e38                                            # finite, and more than an f32 grid can index
    plane = P.copy()
    plane[: n // 2, 2] = 0.25
    calls = {
        "knn": lambda: ne.KDTree3f(P).kNNSearch(P, 8),
        "radius search": lambda: ne.KDTree3f(P).radiusSearch(P, (1.5 * h) ** 2),
        "normals": lambda: ne.NormalEstimation3f(P).getNormalsAndCurvatureKNN(10),
        "kmeans": lambda: clustering.KMeans3f(P).cluster(16, max_iter=5, seed=1),
        "plane ransac": lambda: me.PlaneRANSACEstimator3f(plane).estimate(0.01, n // 2, 40),
        "transform ransac": lambda: me.RigidTransformRANSACEstimator3f(d["dst"], d["src"]).estimate(2.0 * h, n // 2, 40),
        "connected components": lambda: clustering.connected_components(P, (1.2 * h) ** 2),
        "grid downsample": lambda: grid_downsampler.grid_downsample(P, 3.0 * h, normals=d["dst_n"]),
    }
    refused = {
        "knn, k above KNN_MAX_K": lambda: ne.KDTree3f(P).kNNSearch(P, 33),
        "knn, a cloud outside the grid's range": lambda: ne.KDTree3f(far).kNNSearch(far, 8),
    }
    for what, call in calls.items():
        before = live(L)
        call()
        assert live(L) == before, what
    for what, call in refused.items():
        before = live(L)
        with pytest.raises(capi.CilhipError):
            call()
        assert live(L) == before, what
