"""CPU: the yardstick of the map fusion is sound.  tests/_fusion_refs.py holds a literal, one-pixel-at-a-time transcription of the
reference's examples/fusion.cpp:147-236 (with the literal remove() / vec_remove loops) and the vectorised restatement of rules F1-F9 the
GPU tests compare against; here the two are pinned against each other on every class of case the GPU tests run, and the facts DESIGN.md
section 16 quotes about the small scene and tests/golden/frames_full.npz are asserted."""
import numpy as np
import pytest

import _fusion_refs as U
import _projective_refs as R
from test_projective_refs_cpu import GOLDEN, same

F = np.float32
I4 = np.eye(4, dtype=F)
E_SMALL = R.small_E()


def same_model(a, b):
    return all(same(x, y) for x, y in zip(a, b))


def no_borderline_angle(model, frame, pose, K, w, h, prm=None, margin=1e-5):
    """no visited pixel's angle lies within `margin` rad of a threshold it is compared with: no decision hangs on the last bit of an acos"""
    prm = prm or U.Params()
    D = U.decisions(model, frame, pose, K, w, h, prm)
    has = D["has"]
    a, af = D["a"][has].astype(np.float64), D["a_free"][has].astype(np.float64)
    gaps = [np.abs(a - U.threshold(prm.fuse_max_angle_deg)), np.abs(a - U.threshold(prm.append_min_angle_deg)), np.abs(af - U.threshold(prm.free_space_max_angle_deg))]
    return all(not (g[~np.isnan(g)] <= margin).any() for g in gaps)


def random_case(seed, w, h, n_model, n_frame, nan_normals=False, flip=False):
    """a model and a frame that scatter over a w x h image, in front of and behind each other, with several points per pixel"""
    rng = np.random.default_rng(seed)
    K = np.array([[0.8 * max(w, h) + 0.25, 0, (w - 1) / 2], [0, 0.75 * max(w, h) + 0.5, (h - 1) / 2], [0, 0, 1]], F)

    def cloud(n, zs):
        z = rng.choice(np.asarray(zs, F), n).astype(F)
        u, v = rng.uniform(-0.5, w - 0.5, n), rng.uniform(-0.5, h - 0.5, n)
        p = np.stack([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z], axis=1).astype(F)
        nr = rng.normal(0, 0.35, (n, 3)) + np.array([0, 0, -1.0])
        nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
        return p, nr, rng.random((n, 3)).astype(F)

    mp, mn, mc = cloud(n_model, [1.0, 1.004, 1.02, 1.5])
    fp, fn, fc = cloud(n_frame, [1.0, 1.002, 1.2, 1.56])
    if flip:
        mn[::3] = -mn[::3]
    if nan_normals:
        mn[1::4] = np.nan
    conf = rng.uniform(0.5, 4.0, n_model).astype(F)
    return (mp, mn, mc, conf), (fp, fn, fc), K


CASES = [(3, 3, 6, 5), (2, 5, 8, 8), (5, 2, 8, 8), (4, 3, 10, 9), (130, 3, 300, 280), (9, 7, 150, 120), (9, 7, 0, 60)]


@pytest.mark.parametrize("w,h,n_model,n_frame", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("variant", ["identity", "pose", "flipped", "nan-normals"])
def test_restatement_is_the_literal_loop(w, h, n_model, n_frame, variant):
    model, frame, K = random_case(w * 100 + h, w, h, n_model, n_frame, nan_normals=variant == "nan-normals", flip=variant == "flipped")
    pose = E_SMALL if variant == "pose" else I4
    got, cg = U.fuse_frame(model, frame, pose, K, w, h)
    lit, cl = U.fuse_frame_literal(model, frame, pose, K, w, h)
    assert cg == cl and same_model(got, lit)
    assert cg["visited"] == cg["fused"] + cg["appended"] + cg["removed"] + cg["untouched"]
    assert got[0].shape[0] == n_model - cg["removed"] + cg["appended"]
    if w < 3 or h < 3:
        assert cg["visited"] == 0 and same_model(got, model)
    if n_model == 0:
        assert cg["appended"] == cg["visited"] > 0


def test_every_outcome_occurs_in_the_random_cases():
    total = dict.fromkeys(U.NAMES, 0)
    for variant in (False, True):
        model, frame, K = random_case(907, 9, 7, 150, 120, flip=variant)
        for k, v in U.fuse_frame(model, frame, I4, K, 9, 7)[1].items():
            total[k] += v
    assert min(total.values()) > 0, total


def test_nan_weights_are_the_reference_s():
    """conf = 0 under a radial_factor that drives rw to 0: g = 0 / 0 = NaN in both forms"""
    model, frame, K = random_case(907, 9, 7, 150, 120)
    model = model[:3] + (np.zeros_like(model[3]),)
    prm = U.Params(radial_factor=-1e30)
    got, cg = U.fuse_frame(model, frame, I4, K, 9, 7, prm)
    lit, cl = U.fuse_frame_literal(model, frame, I4, K, 9, 7, prm)
    assert cg == cl and same_model(got, lit) and cg["fused"] > 0
    assert np.isnan(got[3]).sum() >= 1 and np.isnan(got[0]).any()


def test_remove_in_closed_form_is_the_literal_loop():
    """F6 against vec_remove on every subset shape that matters: members inside the tail, nothing below n', everything removed, repeats"""
    rng = np.random.default_rng(5)
    for trial in range(3000):
        n = int(rng.integers(1, 15))
        S = rng.integers(0, n, int(rng.integers(0, n + 3)))
        rows = np.arange(n, dtype=F)
        arr = rows.copy()
        n2 = U.remove_rows((arr,), n, S)
        assert arr[:n2].tolist() == [float(v) for v in U.vec_remove_literal(list(range(n)), S.tolist())], (n, S)
    for n, S in ((6, [4, 5]), (6, [3, 5]), (6, [0, 1, 2, 3, 4, 5]), (6, [0, 5]), (6, [2, 2, 2]), (1, [0]), (5, [])):
        arr = np.arange(n, dtype=F)
        n2 = U.remove_rows((arr,), n, np.asarray(S, np.int64))
        assert arr[:n2].tolist() == [float(v) for v in U.vec_remove_literal(list(range(n)), S)]


def test_remove_unstable_restatement_is_the_literal_loop():
    model, _, _ = random_case(3, 9, 7, 150, 10)
    conf = model[3].copy()
    conf[::7] = np.nan      # (a NaN confidence is not below the threshold: it stays)
    model = model[:3] + (conf,)
    for thresh in (0.0, 2.0, 3.0, 100.0, float("nan")):
        got, lit = U.remove_unstable(model, thresh), U.remove_unstable_literal(model, thresh)
        assert same_model(got, lit)
    assert U.remove_unstable(model, 100.0)[3].shape[0] == np.isnan(conf).sum()
    assert U.remove_unstable(model[:3] + (np.ones_like(conf),), 3.0)[0].shape[0] == 0


def test_small_scene_facts():
    """the ray-cast scene (67 x 45, 2 795 model points) against its own points re-rendered from another pose, fused under the identity"""
    model, frame, K, w, h = U.small_scene()
    assert (w, h) == (67, 45) and model[0].shape[0] == 2795
    assert no_borderline_angle(model, frame, I4, K, w, h)
    lit, cl = U.fuse_frame_literal(model, frame, I4, K, w, h)
    assert cl == dict(visited=786, fused=19, appended=8, removed=261, untouched=498)
    got, cg = U.fuse_frame(model, frame, I4, K, w, h)
    assert cg == cl and same_model(got, lit) and got[0].shape[0] == 2795 - 261 + 8
    # removed rows that lie inside the tail [n', n), and holes below it
    D = U.decisions(model, frame, I4, K, w, h, U.Params())
    S = D["m"][D["d"] == U.REMOVE]
    assert 0 < (S >= 2795 - 261).sum() < 261


@pytest.fixture(scope="module")
def full_pair():
    d = np.load(GOLDEN)
    return U.rendered_frame(d["p1"], R.FUSION_K, 640, 480, seed=1), U.rendered_frame(d["p2"], R.FUSION_K, 640, 480, seed=2)


def test_frames_full_facts(full_pair):
    f1, f2 = full_pair
    m1, c1 = U.fuse_frame(U.empty_model(), f1, I4, R.FUSION_K, 640, 480)
    assert c1 == dict(visited=113870, fused=0, appended=113870, removed=0, untouched=0) and same(m1[0], f1[0]) and same(m1[2], f1[2])
    assert no_borderline_angle(m1, f2, I4, R.FUSION_K, 640, 480)
    lit, cl = U.fuse_frame_literal(m1, f2, I4, R.FUSION_K, 640, 480)
    assert cl == dict(visited=115399, fused=58898, appended=10315, removed=1642, untouched=44544)
    got, cg = U.fuse_frame(m1, f2, I4, R.FUSION_K, 640, 480)
    assert cg == cl and same_model(got, lit)
    # the appended confidences are the radial weights: 1 at the principal point's pixels, falling off outwards
    assert m1[3].max() <= 1.0 and m1[3].min() > 0.0


def test_thresholds_evaluate_as_the_reference_writes_them():
    import math

    assert U.threshold(75.0) == 75.0 * math.pi / 180.0 and U.threshold(105.0) == 105.0 * math.pi / 180.0 and U.threshold(45.0) == math.pi / 4
    assert U.ang(np.array([np.nan, 2.0, -2.0, 1.0, 0.0], F)).tolist() == [F(math.pi), 0.0, F(math.pi), 0.0, F(math.pi / 2)]
    assert float(U.Params().radial_factor) == float(F(-0.5) / F(14400))
