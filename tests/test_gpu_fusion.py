"""GPU: map fusion (cilhip_fuse_frame3f, cilhip_fusion_remove_unstable3f and their Python / C++ mirrors) against the numpy restatement of
tests/_fusion_refs.py, bit for bit (NaN matching NaN).  The restatement is pinned against a literal transcription of the reference's loop
by tests/test_fusion_refs_cpu.py, whose case builders are used here.

The splat kernel (k_ic_splat) runs one lane per point in a grid that covers the whole model: it does not stride, so there is no model
"larger than one launch covers" to test."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _fusion_refs as U
import _projective_refs as R
from test_fusion_refs_cpu import CASES, E_SMALL, I4, full_pair, random_case, same_model      # noqa: F401 (full_pair: a fixture)
from test_projective_refs_cpu import same

pytestmark = pytest.mark.gpu

F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


def abi_params(prm):
    from cilantro_amd import capi

    return capi.FusionParams(float(prm.fusion_dist_thresh), float(prm.occlusion_dist_thresh), float(prm.radial_factor), float(prm.fuse_max_angle_deg),
                             float(prm.append_min_angle_deg), float(prm.free_space_max_angle_deg))


def padded(model, capacity, fill=7.0):
    """the model's four arrays with `capacity` rows, the rows behind the model filled with a sentinel"""
    n = model[0].shape[0]
    out = []
    for a in model:
        b = np.full((capacity,) + a.shape[1:], fill, F)
        b[:n] = a
        out.append(b)
    return out


def call_fuse(hip_lib, model, frame, pose, K, w, h, prm=None, device_mem=False, capacity=None):
    """cilhip_fuse_frame3f through ctypes -> (rc, n_out, counts, the four arrays with `capacity` rows after the call)"""
    from cilantro_amd import capi

    prm = prm or U.Params()
    n, nf = model[0].shape[0], frame[0].shape[0]
    capacity = n + min(nf, w * h) if capacity is None else capacity
    arrays = padded(model, capacity)
    fr = [np.ascontiguousarray(a, F) for a in frame]
    if device_mem:
        import torch

        dm, df = [torch.from_numpy(a).cuda() for a in arrays], [torch.from_numpy(a).cuda() for a in fr]
        torch.cuda.synchronize()
        mp, fp, mem = [t.data_ptr() for t in dm], [t.data_ptr() for t in df], capi.MEM_DEVICE
    else:
        mp, fp, mem = [a.ctypes.data for a in arrays], [a.ctypes.data for a in fr], capi.MEM_HOST
    pose_abi, k_abi = np.ascontiguousarray(np.asarray(pose, F).T), np.ascontiguousarray(np.asarray(K, F).T)
    n_out, counts, p = C.c_size_t(0), capi.FusionCounts(), abi_params(prm)
    rc = hip_lib.cilhip_fuse_frame3f(0, mp[0], mp[1], mp[2], mp[3], n, capacity, fp[0], fp[1], fp[2], nf, mem, pose_abi.ctypes.data, k_abi.ctypes.data, w, h, C.byref(p),
                                     C.byref(n_out), C.byref(counts))
    if device_mem:
        arrays = [t.cpu().numpy() for t in dm]
    return rc, n_out.value, {k: int(getattr(counts, k)) for k in U.NAMES}, arrays


def check_fuse(hip_lib, model, frame, pose, K, w, h, prm=None, device_mem=False):
    """one call against the restatement -> the restatement's (model, counts)"""
    want, cw = U.fuse_frame(model, frame, pose, K, w, h, prm)
    rc, n_out, counts, arrays = call_fuse(hip_lib, model, frame, pose, K, w, h, prm, device_mem)
    assert rc == 0, hip_lib.cilhip_last_error(None)
    assert counts == cw and n_out == want[0].shape[0] == model[0].shape[0] - cw["removed"] + cw["appended"]
    for a, b, name in zip(arrays, want, ("points", "normals", "colors", "confidence")):
        assert same(a[:n_out], b), (name, w, h, device_mem)
    return want, cw


@pytest.mark.parametrize("w,h,n_model,n_frame", CASES, ids=lambda v: str(v))
def test_every_shape_and_variant(hip_lib, w, h, n_model, n_frame):
    """3 x 3 (one interior pixel), 2 x 5 and 5 x 2 (none), 4 x 3, 130 x 3 (more than one block in a row), 9 x 7; an empty model; a pose and the
    identity; flipped and NaN model normals; host and device memory"""
    for i, variant in enumerate(("identity", "pose", "flipped", "nan-normals")):
        model, frame, K = random_case(w * 100 + h, w, h, n_model, n_frame, nan_normals=variant == "nan-normals", flip=variant == "flipped")
        pose = E_SMALL if variant == "pose" else I4
        for device_mem in (False, True):
            _, c = check_fuse(hip_lib, model, frame, pose, K, w, h, device_mem=device_mem)
        if w < 3 or h < 3:
            assert c["visited"] == 0
        if (w, h) == (3, 3):
            assert c["visited"] <= 1


def test_flipped_normals_take_the_second_arm_of_append(hip_lib):
    model, frame, K = random_case(907, 9, 7, 150, 120)
    _, plain = check_fuse(hip_lib, model, frame, I4, K, 9, 7)
    flipped = (model[0], (-model[1]).astype(F)) + model[2:]
    D = U.decisions(flipped, frame, I4, K, 9, 7, U.Params())
    assert ((D["d"] == U.APPEND) & D["has"]).sum() > 0      # appended although the pixel has a model point
    _, c = check_fuse(hip_lib, flipped, frame, I4, K, 9, 7, device_mem=True)
    assert c["appended"] > plain["appended"]


def test_small_scene(hip_lib):
    model, frame, K, w, h = U.small_scene()
    for device_mem in (False, True):
        _, c = check_fuse(hip_lib, model, frame, I4, K, w, h, device_mem=device_mem)
    assert c == dict(visited=786, fused=19, appended=8, removed=261, untouched=498)      # (removed rows inside the tail and holes below it: the CPU test)
    check_fuse(hip_lib, model, frame, R.small_E((0.01, -0.02, 0.01), (0.01, 0.0, -0.01)), K, w, h, device_mem=True)


def test_full_frames_once(hip_lib, full_pair):
    f1, f2 = full_pair
    m1, c1 = check_fuse(hip_lib, U.empty_model(), f1, I4, R.FUSION_K, 640, 480, device_mem=True)
    assert c1["appended"] == 113870
    _, c2 = check_fuse(hip_lib, m1, f2, I4, R.FUSION_K, 640, 480, device_mem=True)
    assert c2 == dict(visited=115399, fused=58898, appended=10315, removed=1642, untouched=44544)


def test_nan_weights(hip_lib):
    """conf = 0 under a radial_factor that drives rw to 0: g = 0 / 0"""
    model, frame, K = random_case(907, 9, 7, 150, 120)
    model = model[:3] + (np.zeros_like(model[3]),)
    want, c = check_fuse(hip_lib, model, frame, I4, K, 9, 7, U.Params(radial_factor=-1e30), device_mem=True)
    assert c["fused"] > 0 and np.isnan(want[3]).any() and np.isnan(want[0]).any()


def test_capacity_protocol(hip_lib):
    from cilantro_amd import capi

    model, frame, K, w, h = U.small_scene()
    model = tuple(a[:2600].copy() for a in model)
    want, cw = U.fuse_frame(model, frame, I4, K, w, h)
    need = want[0].shape[0]
    grow = random_case(907, 9, 7, 0, 120)
    want_g, cg = U.fuse_frame(U.empty_model(), grow[1], I4, grow[2], 9, 7)
    assert cg["appended"] > 1
    for device_mem in (False, True):
        # an update that shrinks the model fits in capacity = n_model
        rc, n_out, counts, arrays = call_fuse(hip_lib, model, frame, I4, K, w, h, device_mem=device_mem, capacity=2600)
        assert need < 2600 and rc == capi.OK and n_out == need and all(same(a[:need], b) for a, b in zip(arrays, want))
        # one that grows it does not: the size that is needed, and the four arrays bitwise unchanged
        before = padded(U.empty_model(), cg["appended"] - 1)
        rc, n_out, counts, arrays = call_fuse(hip_lib, U.empty_model(), grow[1], I4, grow[2], 9, 7, device_mem=device_mem, capacity=cg["appended"] - 1)
        assert rc == capi.ERR_INVALID and n_out == cg["appended"] and b"capacity" in hip_lib.cilhip_last_error(None)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(arrays, before))
        rc, n_out, counts, arrays = call_fuse(hip_lib, U.empty_model(), grow[1], I4, grow[2], 9, 7, device_mem=device_mem, capacity=cg["appended"])
        assert rc == capi.OK and n_out == cg["appended"] and all(same(a[:n_out], b) for a, b in zip(arrays, want_g))
    # a model with fused AND removed rows under a short capacity: nothing moved, nothing averaged
    big = random_case(907, 9, 7, 150, 120, flip=True)
    wb, cb = U.fuse_frame(big[0], big[1], I4, big[2], 9, 7)
    assert cb["fused"] > 0 and cb["removed"] > 0 and wb[0].shape[0] > 150
    before = padded(big[0], 150)
    rc, n_out, _, arrays = call_fuse(hip_lib, big[0], big[1], I4, big[2], 9, 7, device_mem=True, capacity=150)
    assert rc == capi.ERR_INVALID and n_out == wb[0].shape[0] and all(a.tobytes() == b.tobytes() for a, b in zip(arrays, before))


def test_4096_model_points_on_one_pixel(hip_lib):
    """a 4 x 3 image: every model point on the ray of interior pixel (2, 1), z drawn from 8 values; the winner is the lowest index among the nearest"""
    rng = np.random.default_rng(11)
    K = np.array([[3.45, 0, 1.5], [0, 3.5, 1.0], [0, 0, 1]], F)
    z = rng.choice(np.linspace(0.75, 1.625, 8).astype(F), 4096).astype(F)
    ray = np.array([(2 - K[0, 2]) / K[0, 0], 0.0, 1.0], F)
    mp = (z[:, None] * ray[None, :]).astype(F)
    mn = np.tile(np.array([0, 0, -1], F), (4096, 1))
    model = (mp, mn, rng.random((4096, 3)).astype(F), rng.uniform(0.5, 2.0, 4096).astype(F))
    for fz, outcome in ((0.752, "fused"), (1.0, "removed"), (0.5, "untouched")):
        frame = ((F(fz) * ray)[None, :].astype(F), np.array([[0, 0, -1]], F), np.array([[0.25, 0.5, 0.75]], F))
        for device_mem in (False, True):
            _, c = check_fuse(hip_lib, model, frame, I4, K, 4, 3, device_mem=device_mem)
        assert c["visited"] == 1 and c[outcome] == 1, (fz, c)


def removal_scene(w, h, extra_first):
    """one model point on the ray of every interior pixel at z = 1, facing the camera, behind `extra_first` points on border pixels; the frame
    sees every pixel at z = 1.5: every interior model point lies in observed free space"""
    K = np.array([[0.8 * max(w, h) + 0.25, 0, (w - 1) / 2], [0, 0.75 * max(w, h) + 0.5, (h - 1) / 2], [0, 0, 1]], F)
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.stack([(xs.reshape(-1) - K[0, 2]) / K[0, 0], (ys.reshape(-1) - K[1, 2]) / K[1, 1], np.ones(w * h)], axis=1)
    inner = ((xs >= 1) & (xs <= w - 2) & (ys >= 1) & (ys <= h - 2)).reshape(-1)
    mp = np.concatenate([rays[~inner][:extra_first], rays[inner]]).astype(F)
    mn = (-mp / np.linalg.norm(mp, axis=1, keepdims=True)).astype(F)
    rng = np.random.default_rng(w * h)
    model = (mp, mn, rng.random(mp.shape).astype(F), rng.uniform(0.5, 2.0, mp.shape[0]).astype(F))
    fp = (1.5 * rays).astype(F)
    frame = (fp, np.tile(np.array([0, 0, -1], F), (w * h, 1)), rng.random(fp.shape).astype(F))
    return model, frame, K, int(inner.sum())


@pytest.mark.parametrize("w,h", [(5, 4), (67, 45)], ids=str)
@pytest.mark.parametrize("device_mem", [False, True])
def test_every_model_point_removed_and_a_removal_with_nothing_below(hip_lib, w, h, device_mem):
    model, frame, K, n_inner = removal_scene(w, h, 0)
    want, c = check_fuse(hip_lib, model, frame, I4, K, w, h, device_mem=device_mem)
    assert c["removed"] == n_inner == model[0].shape[0] and c["appended"] == 0 and want[0].shape[0] == 0      # |S| >= n: cleared
    # the removed rows are exactly the tail [n', n): nothing below n' to fill
    model, frame, K, n_inner = removal_scene(w, h, 7)
    want, c = check_fuse(hip_lib, model, frame, I4, K, w, h, device_mem=device_mem)
    assert c["removed"] == n_inner and want[0].shape[0] == 7 and same(want[0], model[0][:7])
    # ... and with the border points LAST every removed row is a hole below n' filled from the tail, in descending order
    back = tuple(np.concatenate([a[7:], a[:7]]) for a in model)
    want, c = check_fuse(hip_lib, back, frame, I4, K, w, h, device_mem=device_mem)
    assert c["removed"] == n_inner and same(want[0], back[0][-7:][::-1])


def test_remove_unstable(hip_lib):
    from cilantro_amd import capi
    import torch

    model, _, _ = random_case(3, 9, 7, 1500, 10)
    conf = model[3].copy()
    conf[::7] = np.nan
    model = model[:3] + (conf,)
    for thresh in (0.0, 2.0, 3.0, 100.0, float("nan")):
        want = U.remove_unstable(model, thresh)
        for device_mem in (False, True):
            arrays = [a.copy() for a in model]
            held = [torch.from_numpy(a).cuda() for a in arrays] if device_mem else None
            torch.cuda.synchronize()
            ptr = [t.data_ptr() for t in held] if device_mem else [a.ctypes.data for a in arrays]
            n_out = C.c_size_t(77)
            rc = hip_lib.cilhip_fusion_remove_unstable3f(0, ptr[0], ptr[1], ptr[2], ptr[3], 1500, capi.MEM_DEVICE if device_mem else capi.MEM_HOST, thresh, C.byref(n_out))
            assert rc == capi.OK and n_out.value == want[0].shape[0]
            got = [t.cpu().numpy() for t in held] if device_mem else arrays
            assert all(same(g[: n_out.value], w_) for g, w_ in zip(got, want)), (thresh, device_mem)


def sequence():
    """three views of the ray-cast scene and the poses they are fused under: the second registered, the third rendered from elsewhere and
    fused under the identity, so that it removes and appends as well -> (frames, poses, K, w, h)"""
    depth, K = R.raycast_scene()
    w, h = 67, 45
    world = R.depth_to_points(depth, w, h, K, R.Conv(R.U16, 1000.0))[0]
    e1 = R.small_E((0, 0.12, 0), (0.15, 0, 0.02))
    seen_from, poses = [I4, e1, R.small_E((0, 0.25, 0), (0.3, 0, 0.05))], [I4, e1, I4]
    return [U.rendered_frame(world, K, w, h, E, seed=30 + i) for i, E in enumerate(seen_from)], poses, K, w, h


def test_three_frames_in_sequence_then_remove_unstable(hip_lib):
    """the Python mirror, device-resident and grown by doubling, against the restatement run the same way; run twice: the same bits; the
    library's live allocations back to where they started"""
    from cilantro_amd.fusion import SurfelMap3f

    live = (C.c_ulonglong * 2)()
    hip_lib.cilhip_debug_live_allocations(live)
    before = tuple(live)
    frames, poses, K, w, h = sequence()
    want, counts = U.empty_model(), []
    for fr, E in zip(frames, poses):
        want, c = U.fuse_frame(want, fr, E, K, w, h)
        counts.append(c)
    assert counts[0]["appended"] == frames[0][0].shape[0] and all(c["fused"] > 0 for c in counts[1:]) and min(counts[2].values()) > 0
    final = U.remove_unstable(want, 1.2)
    assert 0 < final[0].shape[0] < want[0].shape[0]
    runs = []
    for _ in range(2):
        s = SurfelMap3f()
        assert s.isEmpty() and s.points.shape == (0, 3)
        got_counts = [s.fuse(fr, E, K, w, h) for fr, E in zip(frames, poses)]
        assert got_counts == counts and s.lastCounts() == counts[-1] and s.size() == want[0].shape[0]
        full = [t.cpu().numpy() for t in (s.points, s.normals, s.colors, s.confidence)]
        assert same_model(full, want)
        s.removeUnstable(1.2)
        runs.append([t.cpu().numpy() for t in (s.points, s.normals, s.colors, s.confidence)])
        assert same_model(runs[-1], final)
        assert s.clear().size() == 0
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    hip_lib.cilhip_debug_live_allocations(live)
    assert tuple(live) == before


def test_cpp_mirror_gives_the_python_mirror_results(tmp_path):
    from cilantro_amd.fusion import SurfelMap3f
    from test_components_refs_cpu import build_cpp

    exe = build_cpp(os.path.join(HERE, "cpp", "test_fusion.cpp"), "test_fusion")
    frames, poses, K, w, h = sequence()
    pre = str(tmp_path / "seq")
    np.ascontiguousarray(K.T).tofile(pre + ".K.f32")
    for i, (fr, E) in enumerate(zip(frames, poses)):
        for a, name in zip(fr, ("xyz", "nrm", "rgb")):
            np.ascontiguousarray(a, F).tofile(f"{pre}.f{i}.{name}.f32")
        np.ascontiguousarray(np.asarray(E, F).T).tofile(f"{pre}.f{i}.pose.f32")
    r = subprocess.run([exe, "run", pre, str(w), str(h), str(len(frames)), "1.2"], capture_output=True, text=True)
    assert r.returncode == 0 and "run OK" in r.stdout, r.stdout + r.stderr
    s = SurfelMap3f()
    lines = []
    for i, (fr, E) in enumerate(zip(frames, poses)):
        c = s.fuse(fr, E, K, w, h)
        lines.append("frame %d: visited %d fused %d appended %d removed %d untouched %d" % ((i,) + tuple(c[k] for k in U.NAMES)))
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("frame ")] == lines
    before = [t.cpu().numpy() for t in (s.points, s.normals, s.colors, s.confidence)]
    s.removeUnstable(1.2)
    after = [t.cpu().numpy() for t in (s.points, s.normals, s.colors, s.confidence)]
    for stage, arrays in (("fused", before), ("clean", after)):
        for a, name in zip(arrays, ("points", "normals", "colors", "confidence")):
            assert same(np.fromfile(f"{pre}.{stage}.{name}.f32", F).reshape(a.shape), a), (stage, name)
    assert 0 < after[0].shape[0] < before[0].shape[0]


def test_example_runs_end_to_end(tmp_path):
    """examples/fusion.cpp on frames_full's p1 written as a PLY: 12 views rendered, localised and fused, unstable points removed, PLY out"""
    from test_components_refs_cpu import build_cpp
    from test_projective_refs_cpu import GOLDEN

    exe = build_cpp(os.path.join(os.path.dirname(HERE), "examples", "fusion.cpp"), "example_fusion")
    p1 = np.ascontiguousarray(np.load(GOLDEN)["p1"], F)
    src, out = str(tmp_path / "p1.ply"), str(tmp_path / "model.ply")
    with open(src, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n" % p1.shape[0]).encode())
        f.write(p1.tobytes())
    r = subprocess.run([exe, src, out], capture_output=True, text=True)
    assert r.returncode == 0 and "Fused 12 frames" in r.stdout, r.stdout + r.stderr
    views = [ln for ln in r.stdout.splitlines() if ln.startswith("view ")]
    assert len(views) == 12 and "appended 113870 " in views[0] and all(" fused 0 " not in ln for ln in views[1:])
    kept = int([ln for ln in r.stdout.splitlines() if ln.startswith("Model points:")][0].split(":")[1])
    assert 0 < kept < 113870 + 2000
    with open(out, "rb") as f:
        assert ("element vertex %d" % kept).encode() in f.read(400)
