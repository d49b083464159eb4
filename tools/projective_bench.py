#!/usr/bin/env python
"""Times an ICP iteration of the projective loop (cilhip_set_projection + cilhip_icp_run) beside the grid loop of the same context,
clouds and max_sq_dist, in one run.  The conversions themselves are timed by tools/image_conversions_bench.py.

    python tools/projective_bench.py [--reps 5] [--iters 8] [--out profiles/projective_bench.json]

Cases: tests/golden/frames_full.npz (p2 against p1 with its normals, the fusion camera, 640 x 480) and a synthetic frame of about 1M
points (a ray-cast plane-and-sphere scene at 1184 x 888 unprojected with normals, registered against a slightly displaced copy of itself).
Per case: time per iteration of K iterations with conv_tol = 0 from the same start (the loop's own event time over K, minimum of --reps
after one warm-up) for the projective loop and for the grid loop; the context's grid build (cilhip_get_grid_info, once) is listed
separately with its share of a one-frame registration of K iterations, since a projective-only context still pays it.  The two loops do
not compute the same thing (the associations differ): what is compared is the cost of an iteration.  No ratio is promised or asserted.
Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projective_bench.json"))
    a = ap.parse_args()
    import torch

    import _projective_refs as R
    from cilantro_amd import capi, image_conversions as ic
    from cilantro_amd.icp import Context

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    L = capi.load()
    d = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
    cases = [("frames_full", d["p1"], d["n1"], d["p2"], R.FUSION_K, 640, 480, 0.1 ** 2)]
    w, h = 1184, 888
    K = np.array([[0.82 * w, 0, (w - 1) / 2], [0, 0.82 * w, (h - 1) / 2], [0, 0, 1]], np.float32)
    p, n = ic.depthImageToPointsNormals(R.raycast_scene(w, h, K)[0], ic.DepthValueConverter(1000.0), K)
    move = R.small_E(angles=(0.002, -0.0015, 0.002), t=(0.002, -0.001, 0.0015))
    cases.append(("synthetic_1M", p, n, R.transform(move[:3, :3], move[:3, 3], p), K, w, h, 0.02 ** 2))
    T0 = R.small_E(angles=(0.004, -0.003, 0.005), t=(0.004, -0.003, 0.002))
    results = []
    for name, dst, nrm, src, Kc, cw, ch, r2 in cases:
        ctx = Context(0)
        ctx.set_target(dst, nrm)
        ctx.set_source(src)
        prm = capi.IcpParams()
        L.cilhip_icp_default_params(C.byref(prm))
        prm.metric, prm.w_p2p, prm.w_p2pl, prm.max_iter, prm.conv_tol, prm.max_opt_iter, prm.max_sq_dist = capi.METRIC_COMBINED, 0.0, 1.0, a.iters, 0.0, 1, r2
        row = {"case": name, "n_target": int(dst.shape[0]), "n_source": int(src.shape[0]), "iterations": a.iters, "max_sq_dist": r2,
               "grid_build_ms": float(ctx.grid_info().build_ms)}
        for label, proj in (("grid", None), ("projective", Kc)):
            ctx.set_projection(proj, cw, ch)
            best, ncorr = float("inf"), 0
            for rep in range(a.reps + 1):
                res = ctx.icp_run(prm, T0)
                ms = ctx.last_timing()[0]
                if rep:
                    best = min(best, ms)
                ncorr = int(res.last_ncorr)
            row[label] = {"loop_ms": best, "ms_per_iteration": best / a.iters, "last_ncorr": ncorr}
        row["grid_build_share_of_one_frame_projective"] = row["grid_build_ms"] / (row["grid_build_ms"] + row["projective"]["loop_ms"])
        results.append(row)
        print(json.dumps(row), flush=True)
        ctx.close()
    doc = {"tool": "tools/projective_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "results": results}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
