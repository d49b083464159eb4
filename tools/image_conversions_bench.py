#!/usr/bin/env python
"""Times the image conversions (cilhip_depth_image_to_points3f, cilhip_points_to_depth_image3f, cilhip_points_to_index_map3f through
cilantro_amd.image_conversions) on device-resident arrays, beside the bytes DESIGN.md section 14 says each must move and beside the route
that existed before them in the same run: the conversion on the host (the numpy restatement of tests/_projective_refs.py) plus the
upload of its result.

    python tools/image_conversions_bench.py [--reps 5] [--out profiles/image_conversions_bench.json] [--sizes 640x480,4096x4096]

Per size (a synthetic ray-cast scene in millimetres; 640x480 also as tests/golden/frames_full.npz rendered with the fusion camera) and
conversion: wall time of the call with the stream drained (minimum of --reps after one warm-up; every call creates and destroys its own
stream and scratch buffers, which is part of what a caller pays), the bytes the rules say must move, and the host route's time (once).  These are
whole-call wall times, not kernel times: no rate is derived from them.  No ratio is promised or asserted.  Needs a GPU.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, sync):
    fn()
    sync()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        sync()
        best = min(best, 1e3 * (time.perf_counter() - t0))
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_conversions_bench.json"))
    ap.add_argument("--sizes", default="640x480,4096x4096")
    a = ap.parse_args()
    import torch

    import _projective_refs as R
    from cilantro_amd import image_conversions as ic

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    sync = torch.cuda.synchronize
    conv, rconv = ic.DepthValueConverter(1000.0), R.Conv(R.U16, 1000.0)
    cases = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        K = np.array([[0.82 * w, 0, (w - 1) / 2], [0, 0.82 * w, (h - 1) / 2], [0, 0, 1]], np.float32)
        cases.append((size + " ray-cast", R.raycast_scene(w, h, K)[0], K, w, h))
        if (w, h) == (640, 480):
            p1 = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))["p1"]
            cases.append((size + " frames_full", R.points_to_depth_image(p1, R.FUSION_K, rconv, w, h)[0].reshape(h, w), R.FUSION_K, w, h))
    results = []
    for name, depth, K, w, h in cases:
        npix = w * h
        d_dev = torch.from_numpy(depth.view(np.int16)).cuda()
        row = {"case": name, "pixels": npix}
        for label, normals in (("depth_to_points", False), ("depth_to_points_normals", True)):
            ms, out = timed(lambda: ic.depth_image_to_points(d_dev, conv, K, want_normals=normals), a.reps, sync)
            rows = int(out[0].shape[0])
            moved = 2 * npix + rows * (24 if normals else 12)
            t0 = time.perf_counter()
            ref = R.depth_to_points(depth, w, h, K, rconv, want_normals=normals)
            up = [torch.from_numpy(x).cuda() for x in ref if x is not None]
            sync()
            row[label] = {"rows": rows, "device_ms": ms, "bytes_must_move": moved, "host_route_ms": 1e3 * (time.perf_counter() - t0)}
            assert up[0].shape[0] == rows
        pts = ic.depth_image_to_points(d_dev, conv, K)[0]
        n = int(pts.shape[0])
        pts_host = pts.cpu().numpy()
        for label, fn, per_pixel, ref in (
                ("points_to_index_map", lambda: ic.points_to_index_map(pts, K, w, h), 4, lambda: R.points_to_index_map(pts_host, K, w, h).view(np.int32)),
                ("points_to_depth_image", lambda: ic.points_to_depth_image(pts, K, conv, w, h)[0], 2, lambda: R.points_to_depth_image(pts_host, K, rconv, w, h)[0].view(np.int16))):
            ms, _ = timed(fn, a.reps, sync)
            moved = 12 * n + per_pixel * npix      # every point read once, every pixel written once (the 8-byte keys are scratch on top of that)
            t0 = time.perf_counter()
            up = torch.from_numpy(ref()).cuda()
            sync()
            row[label] = {"points": n, "device_ms": ms, "bytes_must_move": moved, "host_route_ms": 1e3 * (time.perf_counter() - t0)}
            del up
        results.append(row)
        print(json.dumps(row), flush=True)
    doc = {"tool": "tools/image_conversions_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "results": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
