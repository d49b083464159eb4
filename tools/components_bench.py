#!/usr/bin/env python
"""Times connected-component segmentation (cilhip_connected_components3f through cilantro_amd.clustering) beside the yardstick of the
same run: cilhip_radius_search3f on the same cloud and radius -- the call a user had to make for this job before the fused entry existed
(every neighbour list returned to the host, the flood fill still to come).

    python tools/components_bench.py [--reps 5] [--out profiles/components_bench.json] [--cases a,b,...]

Cases: frame_1 after gridDownsample(0.005) with the reference example's parameters (radius 0.02, normals within 2 degrees, segments of
100 points and more), and synthetic surfaces of 1M and 10M points (a wavy height field over the unit square, about one point per
downsample bin, the radius 4 bins).  Per case: the fused call on device-resident inputs with the normals clause and without any
(wall clock around the synchronous call; minimum and median of --reps calls after two warm-up calls), the segments it found, and the
list search (count call + fill call, as its capacity protocol asks; one warm-up, fewer repetitions on the large clouds).  The
expectation written down before any measurement: the fused call is not slower than the list search alone -- it scans the same cells and
writes n words instead of every list.  `fused_over_lists` is that ratio; it is reported, not asserted.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(n, seed=42):
    """n points of z = 0.05 sin(7x) cos(5y) + a step of 0.1 at x = 0.5 over the unit square, with unit normals"""
    from cilantro_amd import synthetic as syn

    u = syn.uniform01(seed, 2 * n).reshape(n, 2).astype(np.float64)
    x, y = u[:, 0], u[:, 1]
    z = 0.05 * np.sin(7 * x) * np.cos(5 * y) + 0.1 * (x > 0.5)
    nrm = np.stack([-0.35 * np.cos(7 * x) * np.cos(5 * y), 0.25 * np.sin(7 * x) * np.sin(5 * y), np.ones(n)], axis=1)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return np.ascontiguousarray(np.stack([x, y, z], axis=1), np.float32), np.ascontiguousarray(nrm, np.float32)


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(min(ms)), float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.json"))
    ap.add_argument("--cases", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/components_bench.py needs a GPU: there is no CPU path to time")
    from cilantro_amd import capi, clustering as cl
    from cilantro_amd import grid_downsampler as gd

    L = capi.load()
    dev = torch.device("cuda:0")
    f = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
    ds = gd.grid_downsample(torch.from_numpy(f["p1"]).to(dev), 0.005, normals=torch.from_numpy(f["n1"]).to(dev))
    cases = [("frame_1_downsampled", ds["points"].cpu().numpy(), ds["normals"].cpu().numpy(), 0.02, 100)]
    for n in (1_000_000, 10_000_000):
        cases.append((f"surface_{n // 1_000_000}m", *surface(n), 4.0 * float(n) ** -0.5, 100))
    only = [c for c in args.cases.split(",") if c]
    angle = np.float32(2.0 * np.pi / 180.0)
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "expectation": "fused_over_lists <= 1 (not asserted)", "cases": {}}
    for name, p, nrm, radius, min_size in cases:
        if only and name not in only:
            continue
        n = p.shape[0]
        r2 = float(np.float32(radius) * np.float32(radius))
        tp, tn = torch.from_numpy(p).to(dev), torch.from_numpy(nrm).to(dev)
        out = {}

        def fused(ev):
            out["r"] = cl.connected_components(tp, r2, ev, min_size, n)

        row = {"points": n, "radius": radius, "min_segment_size": min_size}
        for key, ev in (("normals_2deg", cl.NormalsProximityEvaluator(tn, angle)), ("always_true", None)):
            lo, med = timed(lambda: fused(ev), args.reps)
            off = out["r"][1].cpu().numpy()
            row[key] = {"ms_min": lo, "ms_median": med, "segments": int(off.shape[0] - 1), "largest": int(np.diff(off).max()) if off.shape[0] > 1 else 0}
        # the yardstick: the list search on the same device-resident cloud, lists to the host
        offs = np.zeros(n + 1, np.uint64)
        total = C.c_size_t(0)
        rc = L.cilhip_radius_search3f(0, tp.data_ptr(), n, None, n, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, None, None, 0, C.byref(total))
        if rc != capi.OK:
            raise SystemExit(f"cilhip_radius_search3f (count) failed: {rc}")
        entries = int(total.value)
        idx = np.zeros(max(entries, 1), np.uint32)

        def lists():
            t = C.c_size_t(0)
            for cap, ptr in ((0, None), (entries, idx.ctypes.data)):
                rc = L.cilhip_radius_search3f(0, tp.data_ptr(), n, None, n, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, ptr, None, cap, C.byref(t))
                if rc != capi.OK:
                    raise SystemExit(f"cilhip_radius_search3f failed: {rc}")

        big = n > 2_000_000
        lo, med = timed(lists, 2 if big else args.reps, warm=1)
        row["radius_search_lists"] = {"ms_min": lo, "ms_median": med, "entries": entries, "mean_degree": entries / n - 1.0}
        row["fused_over_lists"] = {k: row[k]["ms_min"] / lo for k in ("normals_2deg", "always_true")}
        result["cases"][name] = row
        print(f"{name:22s} {n:9d} points, radius {radius:.5f} (mean degree {entries / n - 1.0:.1f}): fused {row['normals_2deg']['ms_min']:.2f} ms with the normals clause "
              f"({row['normals_2deg']['segments']} segments), {row['always_true']['ms_min']:.2f} ms without ({row['always_true']['segments']}); list search {lo:.2f} ms "
              f"for {entries} entries -> x{row['fused_over_lists']['normals_2deg']:.3f} / x{row['fused_over_lists']['always_true']:.3f}", flush=True)
        del tp, tn, idx, out
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
