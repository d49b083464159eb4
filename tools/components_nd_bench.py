#!/usr/bin/env python
"""Times connected-component segmentation in dim dimensions (cilhip_connected_components_nd through cilantro_amd.clustering), form 1 (the
exhaustive triangle) and form 2 (sweep and prune), beside, in the same run, the route that existed before it -- cilhip_radius_search_nd
(every neighbour list to the host) + cilhip_connected_components_lists -- and, at dim = 3, cilhip_connected_components3f.

    python tools/components_nd_bench.py [--reps 3] [--out profiles/components_nd_bench.json] [--dims 2,3,6,9,16]
                                        [--cases uniform,blobs,ball] [--sweep 512,1024,...] [--list-cap 150000000]

Method: whole-call wall times on device-resident arrays, the stream drained (every entry returns with its work done), minimum of --reps
after one warm-up.  Clouds:
  uniform  n points uniform in the unit cube, the radius set for a mean degree of about 8 (ignoring the cube's faces), swept over n: where
           pruning gains least, and where form 0's crossover is read off
  blobs    eight unit-variance blobs 50 apart along the first axis, 200 000 points, the radius at the median distance to the 8th neighbour
           of a sample
  ball     every pair inside the radius (one dense component): the union-find's worst case, reported as it comes out
Per row: wall time of forms 1 and 2 with the preparation's, the hook launches' and the tail's share (host clock inside the call:
cilhip_ccn_stats), tile pairs tested / total, launches, segments; form 1's pair rate (pairs / hook time), against which the launch cap of
csrc/components_nd_host.hpp is re-checked; the list route's time, or why it did not run (its lists hold more entries than --list-cap, or
the search refused them).  No ratio is promised or asserted.  Needs a GPU."""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MAX_PAIRS_PER_LAUNCH = 6e10      # CCN_MAX_PAIRS_PER_LAUNCH of csrc/components_nd_host.hpp


def unit_ball_volume(dim):
    return math.pi ** (dim / 2.0) / math.gamma(dim / 2.0 + 1.0)


def uniform_cloud(n, dim, seed=0):
    p = np.random.default_rng(seed).random((n, dim), dtype=np.float32)
    r = (8.0 / (n * unit_ball_volume(dim))) ** (1.0 / dim)
    return p, np.float32(r * r)


def blob_cloud(torch, dim, n=200000, seed=1):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, dim)).astype(np.float32)
    p[:, 0] += 50.0 * rng.integers(0, 8, n).astype(np.float32)
    pd = torch.from_numpy(p).cuda()
    d = torch.cdist(pd[:1024].double(), pd.double())      # (not timed: the fixture's radius)
    r = float(torch.kthvalue(d, 9, dim=1).values.median())      # the 8th neighbour (the point itself is the first value)
    return p, np.float32(r * r)


def ball_cloud(n, dim, seed=2):
    p = (np.random.default_rng(seed).random((n, dim), dtype=np.float32) - np.float32(0.5)) * np.float32(0.5 / math.sqrt(dim))      # diameter <= 0.5
    return p, np.float32(1.0)


def best_of(reps, call):
    best = None
    for rep in range(reps + 1):      # (the first one warms up)
        t0 = time.perf_counter()
        out = call()
        wall = (time.perf_counter() - t0) * 1e3
        if rep and (best is None or wall < best[0]):
            best = (wall, out)      # (out: the call's own copy of whatever it reports beside the result)
    return best


def list_route(L, capi, clustering, pd, n, dim, r2, cap):
    """-> dict(wall_ms, entries, segments) or dict(note): the radius search's two calls, the lists on the host, then the lists entry"""
    t0 = time.perf_counter()
    offs = np.zeros(n + 1, np.uint64)
    total = C.c_size_t(0)
    rc = L.cilhip_radius_search_nd(0, pd.data_ptr(), n, pd.data_ptr(), n, dim, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, None, None, 0, C.byref(total))
    if rc != capi.OK:
        return {"wall_ms": None, "note": "the search refused: " + L.cilhip_last_error(None).decode()}
    if total.value > cap:
        return {"wall_ms": None, "entries": int(total.value), "note": f"not run: the lists hold {total.value} entries (more than --list-cap {cap})"}
    idx = np.zeros(max(int(total.value), 1), np.uint32)
    rc = L.cilhip_radius_search_nd(0, pd.data_ptr(), n, pd.data_ptr(), n, dim, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, idx.ctypes.data, None, int(total.value), C.byref(total))
    if rc != capi.OK:
        return {"wall_ms": None, "entries": int(total.value), "note": "the search refused: " + L.cilhip_last_error(None).decode()}
    out = clustering.connected_components_from_lists(n, offs, idx[: int(total.value)], skip_first=False, symmetric=True)
    return {"wall_ms": (time.perf_counter() - t0) * 1e3, "entries": int(total.value), "segments": int(out[1].shape[0]) - 1}


def measure(args):
    import torch

    from cilantro_amd import capi, clustering

    L = capi.load()
    dims = [int(d) for d in args.dims.split(",")]
    work = []
    for case in args.cases.split(","):
        for dim in dims:
            if case == "uniform":
                work += [(case, dim, n) for n in (int(v) for v in args.sweep.split(","))]
            elif case == "blobs":
                work.append((case, dim, 200000))
            else:
                work += [(case, dim, n) for n in (8192, 30000)]
    rows = []
    for case, dim, n in work:
        p, r2 = uniform_cloud(n, dim) if case == "uniform" else (blob_cloud(torch, dim, n) if case == "blobs" else ball_cloud(n, dim))
        pd = torch.from_numpy(p).cuda()
        torch.cuda.synchronize()
        row = {"case": case, "dim": dim, "n": n, "radius_sq": float(r2)}
        segs = set()
        for form in (1, 2):
            def call(form=form):
                st = {}      # the stats of THIS call, kept with its time
                return clustering.connected_components_nd(pd, float(r2), form=form, stats=st), st

            wall, (out, st) = best_of(args.reps, call)
            row[f"form{form}"] = {"wall_ms": wall, "prep_ms": st["prep_ms"], "hook_ms": st["hook_ms"], "finish_ms": st["finish_ms"], "tiles_tested": st["tiles_tested"],
                                  "tiles_total": st["tiles_total"], "launches": st["launches"], "axis": st["axis"], "segments": int(out[1].shape[0]) - 1}
            segs.add(row[f"form{form}"]["segments"])
        row["form1"]["pairs_per_s"] = (n * (n - 1) / 2.0) / (row["form1"]["hook_ms"] * 1e-3) if row["form1"]["hook_ms"] > 0 else None
        if dim == 3:
            wall, out = best_of(args.reps, lambda: clustering.connected_components(pd, float(r2)))
            row["connected_components3f"] = {"wall_ms": wall, "segments": int(out[1].shape[0]) - 1}
            segs.add(row["connected_components3f"]["segments"])
        lr = best_of(1, lambda: list_route(L, capi, clustering, pd, n, dim, r2, args.list_cap))[1]
        row["list_route"] = lr
        if lr.get("segments") is not None:
            segs.add(lr["segments"])
        if len(segs) != 1:
            raise SystemExit(f"the routes disagree on the segment count: {row}")
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_nd_bench.json"))
    ap.add_argument("--dims", default="2,3,6,9,16")
    ap.add_argument("--cases", default="uniform,blobs,ball")
    ap.add_argument("--sweep", default="512,1024,2048,4096,8192,16384,32768,65536,262144")
    ap.add_argument("--list-cap", type=int, default=150000000)
    args = ap.parse_args()
    rows = measure(args)
    import torch

    rates = [r["form1"]["pairs_per_s"] for r in rows if r["form1"].get("pairs_per_s") and r["n"] >= 30000]      # (below that the launch itself is what is timed)
    result = {"tool": "tools/components_nd_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "rows": rows,
              "launch_cap": {"max_pairs_per_launch": MAX_PAIRS_PER_LAUNCH, "slowest_form1_pairs_per_s_at_n_30000_and_up": min(rates) if rates else None,
                             "seconds_per_full_launch_at_that_rate": MAX_PAIRS_PER_LAUNCH / min(rates) if rates else None}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
