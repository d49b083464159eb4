#!/usr/bin/env python
"""Times the robust (MCD) normal estimation (cilhip_robust_normals_knn3f) beside the plain estimator and beside the route that existed
before it, in one run:

    python tools/robust_normals_bench.py [--reps 5] [--warmup 2] [--out profiles/robust_normals_bench.json] [--large 2000000]

Clouds: frame_1 (tests/golden/frames_full.npz) after gridDownsample(0.005), and the synthetic surface of tools/normals_bench.py (half of
the points on a curved sheet, half uniform in the unit cube).  k = 12, view point at the origin, chi-square threshold 6.25.  Per cloud:
  robust_2_1 / robust_6_3    the robust call at (trials, refinements) = (2, 1) -- the reference example's setting -- and (6, 3), its defaults
  plain                      cilhip_normals_knn3f on the same cloud: search + one covariance per point
  old_route (small cloud)    cilhip_knn3f with the lists sent to the host, then the numpy restatement of the contract (tests/_robust_normal_refs.py)
Every device call works on device-resident arrays (mem = DEVICE: no upload, no download) and returns after its own stream has drained, so
the host clock around the call is the call.  Reported: minimum and median of --reps runs after --warmup runs, in milliseconds, and points
per second at the minimum.  `robust - plain` is what the trials cost on top of the search both share.  No ratio is promised or asserted.
Needs a GPU."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 12
CHI = 6.25


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return {"min_ms": min(ms), "median_ms": float(np.median(ms)), "runs_ms": ms}


def surface(n):
    rng = np.random.default_rng(1)
    x = rng.random((n, 3), dtype=np.float32)
    x[: n // 2, 2] = 0.2 * x[: n // 2, 0] + 0.1 * np.sin(6 * x[: n // 2, 1])
    return x


def bench_cloud(name, x, args, old_route):
    import torch

    from cilantro_amd import capi
    from cilantro_amd.normal_estimation import KDTree3f, NormalEstimation3f, RobustNormalEstimation3f

    n = len(x)
    xd = torch.from_numpy(x).cuda()
    vp = np.zeros(3, np.float32)
    out = {"points": n, "k": K}
    for trials, refinements in ((2, 1), (6, 3)):
        ne = RobustNormalEstimation3f(xd).setViewPoint(vp)
        ne.covarianceMethod().setNumberOfTrials(trials).setNumberOfRefinements(refinements).setChiSquareThreshold(CHI)
        r = timed(lambda: ne._run(K, np.inf, True, True), args.warmup, args.reps)
        nrm = ne._run(K, np.inf, True, True)[0]
        r["invalid_normals"] = int(torch.isnan(nrm).any(dim=1).sum().item())
        r["mpoints_per_s"] = n / r["min_ms"] / 1e3
        out[f"robust_{trials}_{refinements}"] = r
    # the plain estimator, device in -- its outputs are host arrays (the entry's contract), so its download of 16 B per point is inside
    L = capi.load()
    nrm, cur = np.zeros((n, 3), np.float32), np.zeros(n, np.float32)

    def plain():
        rc = L.cilhip_normals_knn3f(0, xd.data_ptr(), n, capi.MEM_DEVICE, K, C.c_float(np.inf), vp.ctypes.data, nrm.ctypes.data, cur.ctypes.data)
        assert rc == capi.OK

    out["plain"] = timed(plain, args.warmup, args.reps)
    out["plain"]["mpoints_per_s"] = n / out["plain"]["min_ms"] / 1e3
    for key in ("robust_2_1", "robust_6_3"):
        out[key]["minus_plain_ms"] = out[key]["min_ms"] - out["plain"]["min_ms"]
    if old_route:
        import _robust_normal_refs as R

        def old(trials, refinements):
            idx, _, cnt = KDTree3f(xd).kNNSearch(None, K)
            return R.robust(x, idx, cnt, trials, refinements, 0.75, CHI, 0)

        for trials, refinements in ((2, 1), (6, 3)):
            r = timed(lambda: old(trials, refinements), 1, max(2, args.reps // 2))
            res = old(trials, refinements)
            ne = RobustNormalEstimation3f(xd).setViewPoint(vp)
            ne.covarianceMethod().setNumberOfTrials(trials).setNumberOfRefinements(refinements).setChiSquareThreshold(CHI)
            mask, inl = ne._run(K, np.inf, False, True)[2:]
            r["decisions_equal_the_device_call"] = bool(np.array_equal(mask.cpu().numpy().view(np.uint32), res.mask) and np.array_equal(inl.cpu().numpy(), res.inlier))
            out[f"old_route_{trials}_{refinements}"] = r
    print(name, json.dumps({k: (v if not isinstance(v, dict) else {a: b for a, b in v.items() if a != "runs_ms"}) for k, v in out.items()}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--large", type=float, default=2e6)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "robust_normals_bench.json"))
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    from cilantro_amd.grid_downsampler import grid_downsample

    p1 = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))["p1"], np.float32)
    small = np.ascontiguousarray(grid_downsample(p1, 0.005)["points"], np.float32)
    res = {"tool": "tools/robust_normals_bench.py", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "reps": args.reps, "chi_square_threshold": CHI,
           "timing": "host clock around a call on device-resident arrays; the call drains its own stream before it returns", "clouds": {}}
    res["clouds"]["frame_1 after gridDownsample(0.005)"] = bench_cloud("frame_1 downsampled", small, args, True)
    res["clouds"]["surface"] = bench_cloud("surface", surface(int(args.large)), args, False)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
