#!/usr/bin/env python
"""Times mean-shift clustering in dim dimensions (cilhip_mean_shift_nd through cilantro_amd.clustering) beside, in the same run, the route
that existed before it -- one cilhip_radius_search_nd per pass for the active seeds (every list to the host), the mean on the host, the
seeds uploaded again with the next search -- and, at dim = 3, cilhip_mean_shift3f.

    python tools/mean_shift_nd_bench.py [--reps 3] [--out profiles/mean_shift_nd_bench.json] [--dims 2,3,6,9,16] [--cases example,self100k,seeds10k]
                                        [--max-iter 10] [--old-passes 2] [--variant TAG=LIBRARY ...]

Cases (flat kernel, radius 2, blobs of tests/_meanshift_nd_refs.unit_blobs_nd's shape): `example`, 3 x 500 points as their own seeds, run
to convergence; `self100k`, 100 000 points as their own seeds; `seeds10k`, 1M points with 10 000 of them as seeds.  The two large cases
stop after --max-iter passes: what is compared is the time per pass.  Per case and dimension: total wall time of the call (minimum of
--reps after one warm-up), the shift passes' and the grouping's share (host clock inside the call: cilhip_msn_stats), passes, rounds,
clusters, the slice counts of the first and the last pass.  The old route is skipped where its lists would hold more than 6e7 entries.

The slice plan's two constants (csrc/mean_shift_nd_host.hpp: the slice cap and the minimum slice length) are swept with --variant: each
names a library built with other values, e.g.
    python -m cilantro_amd.build --tag=_cap32 -DMSN_SLICE_CAP=32
    python tools/mean_shift_nd_bench.py --variant cap32=cilantro_amd/lib/libcilantro_hip_cap32.so
and is timed in a child process of its own (the library is chosen when the package loads).  No ratio is promised or asserted.  Needs a GPU.
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RADIUS, CLUSTER_TOL, CONV_TOL = 2.0, 0.2, 1e-7


def blobs(n, dim, seed=0):
    rng = np.random.default_rng(seed)
    per = n // 3
    p = rng.normal(size=(3 * per, dim)) * min(1.0, 3.0 / dim) ** 0.5
    p[:, dim - 1] += 10.0
    for c in range(3):
        o = rng.normal(size=dim)
        p[c * per:(c + 1) * per] += 2.5 * o / np.linalg.norm(o)
    return np.ascontiguousarray(p[rng.permutation(3 * per)], np.float32)


def old_route(L, capi, torch, points_dev, pts, dim, seeds, passes):
    """-> (ms per pass, mean ball population) or (None, reason)"""
    r2 = np.float32(RADIUS) * np.float32(RADIUS)
    s = seeds.copy()
    n = pts.shape[0]
    active = np.arange(s.shape[0])
    ms, pops = [], []
    for _ in range(passes):
        if active.size == 0:
            break
        t0 = time.perf_counter()
        q = np.ascontiguousarray(s[active])
        qd = torch.from_numpy(q).cuda()      # the upload of the seeds is part of the route
        offs = np.zeros(q.shape[0] + 1, np.uint64)
        total = C.c_size_t(0)
        rc = L.cilhip_radius_search_nd(0, points_dev.data_ptr(), n, qd.data_ptr(), q.shape[0], dim, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, None, None, 0, C.byref(total))
        if rc != capi.OK:
            raise SystemExit(f"cilhip_radius_search_nd failed: {rc}")
        if total.value > 6e7:
            return None, f"skipped: the lists of one pass hold {total.value} entries"
        idx = np.zeros(max(int(total.value), 1), np.uint32)
        rc = L.cilhip_radius_search_nd(0, points_dev.data_ptr(), n, qd.data_ptr(), q.shape[0], dim, capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, idx.ctypes.data, None,
                                       int(total.value), C.byref(total))
        if rc != capi.OK:
            raise SystemExit(f"cilhip_radius_search_nd failed: {rc}")
        o = offs.astype(np.int64)
        cnt = np.diff(o)
        sums = np.add.reduceat(pts[idx[: o[-1]]].astype(np.float64), np.minimum(o[:-1], max(o[-1] - 1, 0)), axis=0) if o[-1] else np.zeros((len(cnt), dim))
        with np.errstate(invalid="ignore", divide="ignore"):
            new = np.where(cnt[:, None] > 0, sums / cnt[:, None], np.nan).astype(np.float32)
        moved = ((new - q) ** 2).sum(axis=1)
        s[active] = new
        active = active[~(moved < np.float32(CONV_TOL) ** 2) & ~np.isnan(new[:, 0])]
        ms.append((time.perf_counter() - t0) * 1e3)
        pops.append(float(cnt.mean()))
    return float(np.min(ms)), float(np.mean(pops))


def measure(args):
    import torch

    from cilantro_amd import capi, clustering

    L = capi.load()
    sizes = {"example": (1500, None, 5000), "self100k": (100000, None, args.max_iter), "seeds10k": (1000000, 10000, args.max_iter)}
    rows = []
    for case in args.cases.split(","):
        n, n_seeds, max_iter = sizes[case]
        for dim in (int(d) for d in args.dims.split(",")):
            p = blobs(n, dim)
            seeds = None if n_seeds is None else np.ascontiguousarray(p[:: n // n_seeds][:n_seeds])
            pd = torch.from_numpy(p).cuda()
            sd = None if seeds is None else torch.from_numpy(seeds).cuda()
            row = {"case": case, "dim": dim, "n": int(p.shape[0]), "n_seeds": int(p.shape[0] if seeds is None else seeds.shape[0]), "max_iter": max_iter}
            best = None
            for rep in range(args.reps + 1):      # (the first one warms up)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = clustering.mean_shift_nd(pd, RADIUS, max_iter, CLUSTER_TOL, CONV_TOL, seeds=sd)
                wall = (time.perf_counter() - t0) * 1e3
                if rep and (best is None or wall < best["wall_ms"]):
                    st = r["stats"]
                    best = {"wall_ms": wall, "shift_ms": st["shift_ms"], "group_ms": st["group_ms"], "passes": st["passes"], "rounds": st["rounds"],
                            "slices_first": st["slices_first"], "slices_last": st["slices_last"], "clusters": int(r["offsets"].shape[0]) - 1,
                            "ms_per_pass": st["shift_ms"] / max(st["passes"], 1)}
            row["nd"] = best
            if not args.child:
                if dim == 3:
                    best3 = None
                    for rep in range(args.reps + 1):
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        r = clustering.mean_shift(pd, RADIUS, max_iter, CLUSTER_TOL, CONV_TOL, seeds=sd)
                        wall = (time.perf_counter() - t0) * 1e3
                        if rep and (best3 is None or wall < best3["wall_ms"]):
                            st = r["stats"]
                            best3 = {"wall_ms": wall, "shift_ms": st["shift_ms"], "group_ms": st["group_ms"], "passes": st["passes"], "rounds": st["rounds"], "form_used": st["form_used"],
                                     "clusters": int(r["offsets"].shape[0]) - 1, "ms_per_pass": st["shift_ms"] / max(st["passes"], 1)}
                    row["mean_shift3f"] = best3
                ms, pop = old_route(L, capi, torch, pd, p, dim, p if seeds is None else seeds, args.old_passes)
                row["old_route"] = {"ms_per_pass": ms, "mean_ball": pop} if ms is not None else {"ms_per_pass": None, "note": pop}
            print(json.dumps(row), flush=True)
            rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_shift_nd_bench.json"))
    ap.add_argument("--dims", default="2,3,6,9,16")
    ap.add_argument("--cases", default="example,self100k,seeds10k")
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--old-passes", type=int, default=2)
    ap.add_argument("--variant", action="append", default=[], help="TAG=LIBRARY: the same cases with another build of the library, in a child process")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rows = measure(args)
    if args.child:
        return
    import torch

    result = {"tool": "tools/mean_shift_nd_bench.py", "device": torch.cuda.get_device_name(0), "reps": args.reps, "radius": RADIUS, "rows": rows, "variants": {}}
    for spec in args.variant:
        tag, lib = spec.split("=", 1)
        env = dict(os.environ, CILHIP_LIB_PATH=os.path.abspath(lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--dims", args.dims, "--cases", args.cases, "--max-iter", str(args.max_iter)],
                           env=env, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"variant {tag} failed:\n{r.stdout}\n{r.stderr}")
        result["variants"][tag] = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
