"""numpy restatements of DESIGN.md section 16 (map fusion of registered depth frames), the yardstick of tests/test_gpu_fusion.py.

Two forms of the update:
  * `fuse_frame_literal` / `remove_unstable_literal`: a per-pixel transcription of the reference's examples/fusion.cpp:147-236 and
    :51-59, run serially with np.float32 scalars, with the literal loops of remove() / vec_remove (utilities/point_cloud.hpp:154-198,
    fusion.cpp:8-33);
  * `fuse_frame` / `remove_unstable`: the vectorised restatement of rules F1-F9 the GPU tests compare against, bit for bit.
tests/test_fusion_refs_cpu.py pins the two against each other.  Both take the index maps and the transforms from
tests/_projective_refs.py and the radial weight from oracle.pinned_expf.

A model is a tuple (xyz (n, 3), normals (n, 3), rgb (n, 3), conf (n,)) of float32 arrays, a frame a tuple (xyz, normals, rgb) in the
camera frame; pose and K are ordinary numpy matrices (pose[r, c], K[r, c])."""
import math

import numpy as np

import _projective_refs as R

F = np.float32
EMPTY = R.EMPTY
FUSE, APPEND, REMOVE, UNTOUCHED = 1, 2, 3, 4
NAMES = ("visited", "fused", "appended", "removed", "untouched")


class Params:
    """cilhip_fusion_params with the reference's values (fusion.cpp:98-100, :192, :211, :223)"""

    def __init__(self, fusion_dist_thresh=0.01, occlusion_dist_thresh=0.025, radial_factor=None, fuse_max_angle_deg=75.0, append_min_angle_deg=105.0,
                 free_space_max_angle_deg=45.0):
        self.fusion_dist_thresh, self.occlusion_dist_thresh = F(fusion_dist_thresh), F(occlusion_dist_thresh)
        self.radial_factor = F(-0.5) / F(120 * 120) if radial_factor is None else F(radial_factor)
        self.fuse_max_angle_deg, self.append_min_angle_deg, self.free_space_max_angle_deg = F(fuse_max_angle_deg), F(append_min_angle_deg), F(free_space_max_angle_deg)


def threshold(deg):
    """F3: T(deg) = ((double)deg * M_PI) / 180.0 -- how 75.0f * M_PI / 180.0f evaluates"""
    return (float(F(deg)) * math.pi) / 180.0


def _expf():
    from oracle import oracle as orc

    return orc.lib().orc_pinned_expf


def radial_weight(x, y, K, radial_factor):
    """F3: rw = pinned_expf(radial_factor * (dx dx + dy dy)), dx = (float)x - K02, dy = (float)y - K12, on arrays of pixel coordinates"""
    K = np.asarray(K, F)
    with np.errstate(all="ignore"):
        dx, dy = np.asarray(x).astype(F) - K[0, 2], np.asarray(y).astype(F) - K[1, 2]
        arg = F(radial_factor) * (dx * dx + dy * dy)
    f = _expf()
    return np.array([f(float(v)) for v in arg.reshape(-1)], F)


def ang(v):
    """F3: (float)acos((double)min(1.0f, max(-1.0f, v))) with std::min / std::max as written (NaN becomes -1)"""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        lo = np.where(F(-1) < v, v, F(-1))
        c = np.where(lo < F(1), lo, F(1)).astype(F)
        return np.arccos(c.astype(np.float64)).astype(F)


def copy_model(model):
    return tuple(np.array(a, F, copy=True) for a in model)


def empty_model():
    return (np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F))


def remove_rows(arrays, n, S):
    """F6 in closed form, in place on the first n rows of every array -> n'"""
    S = np.unique(np.asarray(S, np.int64))
    if S.size == 0:
        return n
    if S.size >= n:
        return 0
    n2 = n - S.size
    holes = S[S < n2]
    tail = np.arange(n2, n)
    survivors = tail[~np.isin(tail, S)][::-1]      # descending: the k-th largest surviving row of [n', n)
    assert survivors.size == holes.size
    for a in arrays:
        a[holes] = a[survivors]
    return n2


def decisions(model, frame, pose, K, w, h, prm):
    """F1-F4 -> dict(k: the visited pixels ascending, f, m, has, d: the decision per visited pixel, a, a_free: the two angles (f32),
    c, nc: model_t)"""
    mx, mn = np.asarray(model[0], F).reshape(-1, 3), np.asarray(model[1], F).reshape(-1, 3)
    fx, fn = np.asarray(frame[0], F).reshape(-1, 3), np.asarray(frame[1], F).reshape(-1, 3)
    pose, K = np.asarray(pose, F), np.asarray(K, F)
    L, t = R.to_cam(pose)
    c, nc = R.transform(L, t, mx), R.linear(L, mn)
    mmap = R.points_to_index_map(mx, K, w, h, pose)
    fmap = R.points_to_index_map(fx, K, w, h)
    if w < 3 or h < 3:
        k = np.zeros(0, np.int64)
    else:
        ys, xs = np.mgrid[1:h - 1, 1:w - 1]
        k = (ys * w + xs).reshape(-1).astype(np.int64)
    k = k[fmap[k] != EMPTY]
    f, m = fmap[k].astype(np.int64), mmap[k].astype(np.int64)
    has = mmap[k] != EMPTY
    mi = np.where(has, m, 0)
    if mx.shape[0] == 0:
        c, nc = np.zeros((1, 3), F), np.zeros((1, 3), F)      # (never read: has is false everywhere)
    with np.errstate(all="ignore"):
        fz, mz = fx[f, 2], c[mi, 2]
        a = ang(R.dot3(nc[mi, 0], nc[mi, 1], nc[mi, 2], fn[f, 0], fn[f, 1], fn[f, 2]))
        a64 = a.astype(np.float64)
        fuse = has & (np.abs(mz - fz) < prm.fusion_dist_thresh) & (a64 < threshold(prm.fuse_max_angle_deg))
        alone = ~has & (mmap[k - 1] == EMPTY) & (mmap[k + 1] == EMPTY) & (mmap[k - w] == EMPTY) & (mmap[k + w] == EMPTY)
        append = ~fuse & (alone | (has & (a64 > threshold(prm.append_min_angle_deg))))
        cn = R.normalized(c[mi])
        a_free = ang(-R.dot3(cn[:, 0], cn[:, 1], cn[:, 2], nc[mi, 0], nc[mi, 1], nc[mi, 2]))
        remove = ~fuse & ~append & has & (fz > mz + prm.occlusion_dist_thresh) & (a_free.astype(np.float64) < threshold(prm.free_space_max_angle_deg))
    d = np.full(k.size, UNTOUCHED, np.uint8)
    d[fuse], d[append], d[remove] = FUSE, APPEND, REMOVE
    return dict(k=k, f=f, m=m, has=has, d=d, a=a, a_free=a_free, fz=fz, mz=mz)


def counts_of(d):
    n = [int((d == v).sum()) for v in (FUSE, APPEND, REMOVE, UNTOUCHED)]
    return dict(zip(NAMES, [sum(n)] + n))


def fuse_frame(model, frame, pose, K, w, h, prm=None):
    """F1-F8 -> (the model after the update, counts)"""
    prm = prm or Params()
    mx, mn, mc, conf = copy_model(model)
    mx, mn, mc = mx.reshape(-1, 3), mn.reshape(-1, 3), mc.reshape(-1, 3)
    fx, fn, fc = (np.asarray(a, F).reshape(-1, 3) for a in frame)
    pose, K = np.asarray(pose, F), np.asarray(K, F)
    n = mx.shape[0]
    if w * h == 0 or fx.shape[0] == 0:
        return (mx, mn, mc, conf), dict(zip(NAMES, [0] * 5))
    D = decisions((mx, mn, mc, conf), (fx, fn, fc), pose, K, w, h, prm)
    k, f, m, d = D["k"], D["f"], D["m"], D["d"]
    rw = np.zeros(k.size, F)
    need = (d == FUSE) | (d == APPEND)
    rw[need] = radial_weight(k[need] % w, k[need] // w, K, prm.radial_factor)
    q, nq = R.transform(pose[:3, :3], pose[:3, 3], fx[f]), R.linear(pose[:3, :3], fn[f])
    # F5 (a model point wins at most one pixel: no ordering between pixels)
    s = d == FUSE
    ms = m[s]
    assert np.unique(ms).size == ms.size
    with np.errstate(all="ignore"):
        g = rw[s] / (rw[s] + conf[ms])
        gc = F(1) - g
        mx[ms] = gc[:, None] * mx[ms] + g[:, None] * q[s]
        mn[ms] = R.normalized((gc[:, None] * mn[ms] + g[:, None] * nq[s]).astype(F))
        mc[ms] = gc[:, None] * mc[ms] + g[:, None] * fc[f[s]]
        conf[ms] = conf[ms] + g
    # F6, F7
    n2 = remove_rows((mx, mn, mc, conf), n, m[d == REMOVE])
    s = d == APPEND
    out = (np.concatenate([mx[:n2], q[s]]), np.concatenate([mn[:n2], nq[s]]), np.concatenate([mc[:n2], fc[f[s]]]), np.concatenate([conf[:n2], rw[s]]))
    return tuple(np.ascontiguousarray(a, F) for a in out), counts_of(d)


def remove_unstable(model, conf_thresh):
    """F9 -> the model after cleanup_callback"""
    mx, mn, mc, conf = copy_model(model)
    with np.errstate(all="ignore"):
        S = np.flatnonzero(conf < F(conf_thresh))
    n2 = remove_rows((mx, mn, mc, conf), conf.shape[0], S)
    return mx[:n2].copy(), mn[:n2].copy(), mc[:n2].copy(), conf[:n2].copy()


# ---- the reference's loops, one element at a time ----------------------------------------------------------------------
def vec_remove_literal(vec, indices):
    """fusion.cpp:8-33 on a Python list (point_cloud.hpp:154-198 is the same loop over the cloud's columns)"""
    if len(indices) == 0:
        return vec
    indices_set = set(int(i) for i in indices)
    if len(indices_set) >= len(vec):
        return []
    valid_ind = len(vec) - 1
    while valid_ind in indices_set:
        valid_ind -= 1
    ordered = sorted(indices_set)
    it = 0
    while it < len(ordered) and ordered[it] < valid_ind:
        vec[ordered[it]], vec[valid_ind] = vec[valid_ind], vec[ordered[it]]
        valid_ind -= 1
        while ordered[it] < valid_ind and valid_ind in indices_set:
            valid_ind -= 1
        it += 1
    return vec[: valid_ind + 1]


def _ang_s(v):
    lo = v if F(-1) < v else F(-1)       # std::max(-1.0f, v)
    c = lo if lo < F(1) else F(1)        # std::min(1.0f, .)
    return F(math.acos(float(c)))


def fuse_frame_literal(model, frame, pose, K, w, h, prm=None):
    """:147-236 serially -> (the model after the update, counts)"""
    prm = prm or Params()
    mx, mn, mc, conf = copy_model(model)
    mx, mn, mc = mx.reshape(-1, 3), mn.reshape(-1, 3), mc.reshape(-1, 3)
    fx, fn, fc = (np.asarray(a, F).reshape(-1, 3) for a in frame)
    pose, K = np.asarray(pose, F), np.asarray(K, F)
    cnt = dict(zip(NAMES, [0] * 5))
    if w * h == 0 or fx.shape[0] == 0:
        return (mx, mn, mc, conf), cnt
    expf = _expf()
    frame_t_p, frame_t_n = R.transform(pose[:3, :3], pose[:3, 3], fx), R.linear(pose[:3, :3], fn)      # :151
    L, t = R.to_cam(pose)
    model_t_p, model_t_n = R.transform(L, t, mx), R.linear(L, mn)                                      # :152
    mmap = R.points_to_index_map(mx, K, w, h, pose)                                                    # :156 (the map of model_t)
    fmap = R.points_to_index_map(fx, K, w, h)                                                          # :158
    t_fuse, t_append, t_free = threshold(prm.fuse_max_angle_deg), threshold(prm.append_min_angle_deg), threshold(prm.free_space_max_angle_deg)
    app, remove_ind = [], []
    with np.errstate(all="ignore"):
        for y in range(1, h - 1):
            for x in range(1, w - 1):
                fi, mi = int(fmap[y * w + x]), int(mmap[y * w + x])
                if fi == EMPTY:
                    continue
                cnt["visited"] += 1
                frame_depth = fx[fi, 2]
                model_depth = model_t_p[mi, 2] if mi != EMPTY else F(0)
                dx, dy = F(F(x) - K[0, 2]), F(F(y) - K[1, 2])
                rw = F(expf(float(F(prm.radial_factor * F(F(dx * dx) + F(dy * dy))))))
                a = _ang_s(R._dot_s(model_t_n[mi], fn[fi])) if mi != EMPTY else None
                if mi != EMPTY and abs(F(model_depth - frame_depth)) < prm.fusion_dist_thresh and float(a) < t_fuse:
                    wgt = F(rw / F(rw + conf[mi]))
                    wc = F(F(1) - wgt)
                    mx[mi] = wc * mx[mi] + wgt * frame_t_p[fi]
                    v = (wc * mn[mi] + wgt * frame_t_n[fi]).astype(F)
                    z = R._dot_s(v, v)
                    mn[mi] = v / np.sqrt(z) if z > 0 else v
                    mc[mi] = wc * mc[mi] + wgt * fc[fi]
                    conf[mi] = F(conf[mi] + wgt)
                    cnt["fused"] += 1
                elif (mi == EMPTY and mmap[y * w + x - 1] == EMPTY and mmap[y * w + x + 1] == EMPTY and mmap[(y - 1) * w + x] == EMPTY and mmap[(y + 1) * w + x] == EMPTY) or \
                        (mi != EMPTY and float(a) > t_append):
                    app.append((frame_t_p[fi], frame_t_n[fi], fc[fi], rw))
                    cnt["appended"] += 1
                else:
                    free = False
                    if mi != EMPTY and frame_depth > F(model_depth + prm.occlusion_dist_thresh):
                        p = model_t_p[mi]
                        z = R._dot_s(p, p)
                        pn = (p / np.sqrt(z)).astype(F) if z > 0 else p
                        free = float(_ang_s(-R._dot_s(pn, model_t_n[mi]))) < t_free
                    if free:
                        remove_ind.append(mi)
                        cnt["removed"] += 1
                    else:
                        cnt["untouched"] += 1
    keep = vec_remove_literal(list(range(mx.shape[0])), remove_ind)                                    # :229-230
    keep = np.asarray(keep, np.int64)
    arr = lambda rows, width: np.array(rows, F).reshape((-1, width) if width else (-1,))      # noqa: E731
    out = (np.concatenate([mx[keep], arr([r[0] for r in app], 3)]), np.concatenate([mn[keep], arr([r[1] for r in app], 3)]),
           np.concatenate([mc[keep], arr([r[2] for r in app], 3)]), np.concatenate([conf[keep], arr([r[3] for r in app], 0)]))
    return tuple(np.ascontiguousarray(a, F) for a in out), cnt


def remove_unstable_literal(model, conf_thresh):
    """:51-59"""
    mx, mn, mc, conf = copy_model(model)
    with np.errstate(all="ignore"):
        remove_ind = [i for i in range(conf.shape[0]) if conf[i] < F(conf_thresh)]
    keep = np.asarray(vec_remove_literal(list(range(conf.shape[0])), remove_ind), np.int64)
    return mx[keep], mn[keep], mc[keep], conf[keep]


# ---- scenes ---------------------------------------------------------------------------------------------------------------------
def rendered_frame(xyz, K, w, h, E=None, scale=1000.0, seed=0):
    """a cloud rendered to a u16 depth image from camera pose E and read back with normals (fromRGBDImages), with colours drawn from `seed`
    -> (xyz, normals, rgb) in the camera frame"""
    conv = R.Conv(R.U16, scale)
    depth, _ = R.points_to_depth_image(xyz, K, conv, w, h, E)
    rgb = np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    P, N, C = R.depth_to_points(depth, w, h, K, conv, rgb=rgb, want_normals=True)
    return P, N, C


def small_scene():
    """the ray-cast plane-and-sphere scene (67 x 45) as a model with unit confidences, and the model's points re-rendered from
    small_E((0, 0.25, 0), (0.3, 0, 0.05)) as the frame, to be fused under the IDENTITY pose -> (model, frame, K, w, h)"""
    depth, K = R.raycast_scene()
    w, h = 67, 45
    conv = R.Conv(R.U16, 1000.0)
    rgb = np.random.default_rng(21).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    P, N, C = R.depth_to_points(depth, w, h, K, conv, rgb=rgb, want_normals=True)
    frame = rendered_frame(P, K, w, h, R.small_E((0, 0.25, 0), (0.3, 0, 0.05)), seed=22)
    conf = np.ones(P.shape[0], F)
    return (P, N, C, conf), frame, K, w, h
