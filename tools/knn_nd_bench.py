#!/usr/bin/env python
"""Times the exhaustive N-D neighbour search (cilhip_knn_nd / cilhip_radius_search_nd through cilantro_amd.kd_tree).

    python tools/knn_nd_bench.py [--reps 3] [--out profiles/knn_nd_bench.json] [--cases frame,synthetic] [--clock-ghz 2.4]

One process, device-resident inputs; every figure is the wall time of the whole call with the stream drained, minimum of --reps after a warm-up.
  frame      the downsampled frame_1 (tests/golden/frame1_c1.npz, 15 531 points) as 3-, 6- and 9-D features: points, points + normals, points +
             normals + colours (the fixture carries no colours: a smooth function of the position stands in for them)
  synthetic  100 000 standard normal points in 2, 3, 6, 9 and 16 dimensions
Per cloud: self k-NN at k = 10 and 30, and one radius search at a radius that gives about 30 neighbours (the median 30th distance of the k-NN
run).  Beside each row, for context only: cilhip_knn3f on the same cloud where dim = 3, and scipy.spatial.cKDTree.query (k = 10, 16 workers) on
the same points in the same process.  Reported: candidate pairs per second, and that rate as a fraction of the vector-ALU bound
    256 CUs x 4 SIMDs x 64 lanes x clock / (2 cycles x vector instructions per pair)
with the kernel's own count of vector instructions per pair in its inner loop (read off the disassembly: 2 * dim with the packed forms the
compiler chooses) and --clock-ghz.  No ratio is promised or asserted.  Needs a GPU."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_nd_bench.json"))
    ap.add_argument("--cases", default="frame,synthetic")
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--scipy-max-dim", type=int, default=16)
    ap.add_argument("--no-context", action="store_true", help="leave out the grid search and scipy (a run under a profiler)")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/knn_nd_bench.py needs a GPU: there is no CPU path to time")
    from scipy.spatial import cKDTree

    from cilantro_amd import kd_tree
    from cilantro_amd import normal_estimation as ne
    from spectral_bench import best

    doc = {"tool": "tools/knn_nd_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "clock_ghz_assumed": a.clock_ghz, "rows": []}

    def timed(fn):
        def run():
            r = fn()
            torch.cuda.synchronize()
            return r
        return best(run, a.reps)

    clouds = []
    if "frame" in a.cases:
        f = np.load(os.path.join(ROOT, "tests", "golden", "frame1_c1.npz"))
        p, n = f["dst"], f["dst_n"]
        c = (0.5 + 0.5 * np.sin(4.0 * p + np.array([0.0, 2.0, 4.0]))).astype(np.float32)      # stand-in colours
        clouds += [("frame_1_downsampled", 3, p), ("frame_1_downsampled", 6, np.concatenate([p, n], 1)), ("frame_1_downsampled", 9, np.concatenate([p, n, c], 1))]
    if "synthetic" in a.cases:
        rng = np.random.default_rng(16)
        full = rng.standard_normal((100_000, 16)).astype(np.float32)
        clouds += [("synthetic_100k", d, np.ascontiguousarray(full[:, :d])) for d in (2, 3, 6, 9, 16)]

    for name, dim, pts in clouds:
        pts = np.ascontiguousarray(pts, np.float32)
        n = len(pts)
        dev = torch.from_numpy(pts).cuda()
        torch.cuda.synchronize()
        tree = kd_tree.KDTreeXf(dev)
        pairs = float(n) * float(n)
        bound = 256 * 4 * 64 * a.clock_ghz * 1e9 / (2.0 * 2.0 * dim)
        row = {"cloud": name, "n": n, "dim": dim, "valu_instructions_per_pair": 2 * dim, "valu_bound_pairs_per_s": bound}
        d30 = None
        for k in (10, 30):
            ms, (idx, d2, cnt) = timed(lambda: tree.kNNSearch(None, k))
            row[f"knn_k{k}"] = {"wall_ms": ms, "pairs_per_s": pairs / (ms * 1e-3), "fraction_of_valu_bound": pairs / (ms * 1e-3) / bound}
            if k == 30:
                d30 = float(np.median(d2[:, 29]))
        ms, (off, ridx, rd2) = timed(lambda: tree.radiusSearch(None, d30))
        row["radius"] = {"radius_sq": d30, "mean_neighbours": float(off[-1]) / n, "wall_ms": ms, "pairs_per_s": 2 * pairs / (ms * 1e-3),
                         "fraction_of_valu_bound": 2 * pairs / (ms * 1e-3) / bound, "note": "two passes over the pairs (count, fill), one sort"}
        if dim == 3 and not a.no_context:
            grid = ne.KDTree3f(dev)
            for k in (10, 30):
                ms, _ = timed(lambda: grid.kNNSearch(None, k))
                row[f"knn3f_grid_k{k}_wall_ms"] = ms
            ms, _ = timed(lambda: grid.radiusSearch(None, d30))
            row["radius_search3f_grid_wall_ms"] = ms
        if dim <= a.scipy_max_dim and not a.no_context:
            t0 = time.perf_counter()
            sp = cKDTree(pts)
            build_ms = 1e3 * (time.perf_counter() - t0)
            nq = n if dim <= 9 else min(n, 10_000)      # (a kd-tree prunes little in 16 dimensions: a tenth of the queries)
            t0 = time.perf_counter()
            sp.query(pts[:nq], k=10, workers=16)
            row["scipy_cKDTree_k10"] = {"build_ms": build_ms, "n_queries": nq, "query_ms": 1e3 * (time.perf_counter() - t0), "workers": 16}
        print(json.dumps(row), flush=True)
        doc["rows"].append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:      # (after every row: a run that is cut short keeps what it measured)
            json.dump(doc, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
