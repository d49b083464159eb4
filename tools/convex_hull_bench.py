#!/usr/bin/env python
"""Times the convex hull and the polytope queries (cilhip_convex_hull_create, cilhip_polytope(s)_* through cilantro_amd.spatial).

    python tools/convex_hull_bench.py [--reps 3] [--out profiles/convex_hull_bench.json] [--cases gauss_1m,gauss_10m,ball_1m,frame_1_downsampled]

Clouds: Gaussian with 1M and 10M points, a solid ball (uniform in the unit ball, 1M), frame_1 after gridDownsample(0.005); device-resident.
Per cloud:
  hull      ConvexHull3f(points, True, True): the whole call as a wall time with the stream drained (minimum of --reps after one warm-up), its
            rounds, the survivors per round, the plane tests, and k_hull_cull by device events (CILHIP_HULL_TIMING=1, a run of its own)
  scipy     scipy.spatial.ConvexHull on the f64 image of the same points, in the same run (one run; host memory)
  queries   the signed distances (12 facets only: the output is F x n), the mask and the indices of the same cloud against a 12-facet polytope
            (the hull of 8 of its points) and a 6000-facet one (the hull of 3000 points on a sphere that cuts the cloud): wall times with the
            stream drained, minimum of --reps
and once the float4 copy rate of the same run.  No ratio is promised or asserted.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convex_hull_bench.json"))
    ap.add_argument("--cases", default="gauss_1m,gauss_10m,ball_1m,frame_1_downsampled")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/convex_hull_bench.py needs a GPU: there is no CPU path to time")
    from scipy.spatial import ConvexHull

    from cilantro_amd import grid_downsampler as gd
    from cilantro_amd import spatial
    from spectral_bench import best, copy_rate

    rate = copy_rate(torch)
    doc = {"tool": "tools/convex_hull_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "float4_copy_bytes_per_s": rate, "results": {}}

    def cloud(name):
        rng = np.random.default_rng(len(name))
        if name.startswith("gauss"):
            return rng.standard_normal((10_000_000 if name.endswith("10m") else 1_000_000, 3)).astype(np.float32)
        if name == "ball_1m":
            g = rng.standard_normal((1_000_000, 3))
            return (g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0, 1, (1_000_000, 1)) ** (1.0 / 3.0)).astype(np.float32)
        f = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
        return gd.grid_downsample(torch.from_numpy(f["p1"]).cuda(), 0.005)["points"].cpu().numpy()

    def timed(fn):
        def run():
            r = fn()
            torch.cuda.synchronize()
            return r
        return best(run, a.reps)

    for name in [c for c in a.cases.split(",") if c]:
        pts = cloud(name)
        n = len(pts)
        dev = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        ms, hull = timed(lambda: spatial.ConvexHull3f(dev, True, True))
        os.environ["CILHIP_HULL_TIMING"] = "1"
        timed_hull = spatial.ConvexHull3f(dev, True, True)
        del os.environ["CILHIP_HULL_TIMING"]
        t0 = time.perf_counter()
        sp = ConvexHull(pts.astype(np.float64))
        scipy_ms = 1e3 * (time.perf_counter() - t0)
        res = {"n": n, "hull": {"wall_ms": ms, "rounds": hull.info_["rounds"], "survivors_per_round": [int(v) for v in hull.survivors_per_round_], "plane_tests": hull.info_["plane_tests"],
                                "k_hull_cull_ms": timed_hull.info_["cull_ms"], "n_vertices": hull.info_["n_vertices"], "n_facets": hull.info_["n_facets"], "area": hull.getArea(),
                                "volume": hull.getVolume(), "points_bytes_over_wall_fraction_of_copy_rate": 12.0 * n / (ms * 1e-3) / rate},
               "scipy": {"wall_ms": scipy_ms, "n_vertices": int(len(sp.vertices)), "n_facets": int(len(sp.simplices)), "area": float(sp.area), "volume": float(sp.volume),
                         "same_vertices": bool(np.array_equal(np.sort(sp.vertices), hull.getVertexPointIndices()))}}
        # the two query polytopes: 12 facets (the hull of 8 of the cloud's points), about 6000 (3000 points on a sphere through the cloud)
        centre, spread = pts.mean(axis=0), pts.std(axis=0).mean()
        rng = np.random.default_rng(3)
        g = rng.standard_normal((3000, 3))
        shell = (centre + 1.2 * spread * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
        box = (centre + spread * np.array([[x, y, z] for x in (-1, 1) for y in (-1.1, 1) for z in (-1, 1.2)]) * (1 + 0.05 * rng.uniform(size=(8, 1)))).astype(np.float32)
        queries = {}
        for label, src in (("facets_12", box), ("facets_6000", shell)):
            poly = spatial.ConvexHull3f(src, True, True)
            q = {"n_facets": poly.info_["n_facets"]}
            q["mask_ms"], mask = timed(lambda: poly.getInteriorPointsIndexMask(dev))
            q["indices_ms"], idx = timed(lambda: poly.getInteriorPointIndices(dev))
            q["inside"] = int(mask.sum().item())
            assert q["inside"] == int(idx.numel())
            if label == "facets_12":
                q["signed_distances_ms"], _ = timed(lambda: poly.getPointSignedDistancesFromFacets(dev))
            q["points_bytes_over_mask_fraction_of_copy_rate"] = 12.0 * n / (q["mask_ms"] * 1e-3) / rate
            queries[label] = q
        res["queries"] = queries
        doc["results"][name] = res
        print(name, json.dumps(res), flush=True)
        del dev
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
