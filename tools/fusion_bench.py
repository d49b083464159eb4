#!/usr/bin/env python
"""Times the map fusion (cilhip_fuse_frame3f through cilantro_amd.fusion) on device-resident arrays at 640x480, for models of about 1e5,
1e6 and 1e7 points, beside the route that existed before it in the same run: the model downloaded, the update made on the host (the
vectorised numpy restatement of tests/_fusion_refs.py), the model uploaded again.

    python tools/fusion_bench.py [--reps 5] [--out profiles/fusion_bench.json] [--layers 1,9,88]

The model is tests/golden/frames_full.npz's p1 rendered with the fusion camera and read back with normals (113 870 points, the first
frame fused into an empty model), the frame is p2 treated the same way, the pose the identity.  Larger models add layers of the same
points pushed back along their rays (factor 1.05, 1.10, ...): they project to the same pixels and lose them to the first layer, so the
decisions stay close to those of the small model (the counts are recorded) and mostly the projection pass grows.  Per model: wall time of the whole call with the stream
drained (minimum of --reps after one warm-up; the call creates and destroys its own stream and scratch, which is part of what a caller
pays; the model is restored from a device copy outside the timed window), the counts, and the host route's time (once).  Whole-call wall
times, not kernel times: no rate is derived from them.  No ratio is promised or asserted.  Needs a GPU.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fusion_bench.json"))
    ap.add_argument("--layers", default="1,9,88")
    a = ap.parse_args()
    import torch

    import _fusion_refs as U
    import _projective_refs as R
    from cilantro_amd import fusion

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    sync = torch.cuda.synchronize
    w, h, K, pose = 640, 480, R.FUSION_K, np.eye(4, dtype=np.float32)
    d = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
    f1, f2 = U.rendered_frame(d["p1"], K, w, h, seed=1), U.rendered_frame(d["p2"], K, w, h, seed=2)
    base, _ = U.fuse_frame(U.empty_model(), f1, pose, K, w, h)
    frame_dev = tuple(torch.from_numpy(x).cuda() for x in f2)
    nf = f2[0].shape[0]
    results = []
    for layers in (int(v) for v in a.layers.split(",")):
        scale = (1.0 + 0.05 * np.arange(layers)).astype(np.float32)
        model = (np.concatenate([base[0] * s for s in scale]), np.tile(base[1], (layers, 1)), np.tile(base[2], (layers, 1)), np.tile(base[3], layers))
        n = model[0].shape[0]
        cap = n + min(nf, w * h)
        pristine = [torch.empty((cap,) + x.shape[1:], dtype=torch.float32, device="cuda") for x in model]
        for t, x in zip(pristine, model):
            t[:n] = torch.from_numpy(x).cuda()
        work = [t.clone() for t in pristine]
        best, n_out, counts = float("inf"), 0, None
        for rep in range(a.reps + 1):
            for t, p in zip(work, pristine):
                t.copy_(p)
            sync()
            t0 = time.perf_counter()
            n_out, counts = fusion.fuse_frame(work, n, frame_dev, pose, K, w, h)      # (returns with its stream drained)
            ms = 1e3 * (time.perf_counter() - t0)
            if rep:
                best = min(best, ms)
        # the route without the entry: download, numpy, upload
        sync()
        t0 = time.perf_counter()
        host = tuple(t[:n].cpu().numpy() for t in pristine)
        t1 = time.perf_counter()
        want, cw = U.fuse_frame(host, f2, pose, K, w, h)
        t2 = time.perf_counter()
        up = [torch.from_numpy(x).cuda() for x in want]
        sync()
        t3 = time.perf_counter()
        agree = cw == counts and n_out == want[0].shape[0] and all(torch.equal(t[:n_out].nan_to_num(7.0), u_.nan_to_num(7.0)) for t, u_ in zip(work, up))
        row = {"model_points": n, "frame_points": nf, "n_out": n_out, "counts": counts, "device_ms": best,
               "host_route_ms": {"download": 1e3 * (t1 - t0), "numpy_update": 1e3 * (t2 - t1), "upload": 1e3 * (t3 - t2), "total": 1e3 * (t3 - t0)},
               "device_result_equals_host_route": bool(agree)}
        results.append(row)
        print(json.dumps(row), flush=True)
        del pristine, work, up
    doc = {"tool": "tools/fusion_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "image": "640x480", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
