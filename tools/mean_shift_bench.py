#!/usr/bin/env python
"""Times mean-shift clustering (cilhip_mean_shift3f through cilantro_amd.clustering) per shift form, beside the route that existed before it
in the same run: one cilhip_radius_search3f per pass for the active seeds (every list to the host), the weighted mean on the host, the
seeds uploaded again with the next search.

    python tools/mean_shift_bench.py [--reps 3] [--out profiles/mean_shift_bench.json] [--cases a,b,...] [--old-passes 3]

Cases: the reference example's (3 x 500 N(0, 1) points, radius 2, every point a seed, flat kernel); frame_1 after gridDownsample(0.005)
as its own seeds at radius 0.02; a 1M-point synthetic surface with 10 000 of its points as seeds at radius 0.02.  The two large cases
stop after --max-iter passes (default 30): what is compared is the time per pass.  Per case and form (1: a lane per seed, 2: a wave per
seed; 0: what the code picks, with the ball population it estimated): total wall time of the call (minimum of --reps after one warm-up),
the shift passes' and the grouping's share (host clock inside the call), passes, rounds, clusters.  `wave_over_lane` is the per-pass
ratio: the crossover of the two forms in ball population is read off these cases and written into NOTEBOOK.md beside
MS_WAVE_FORM_MIN_BALL (cilantro_amd/csrc/mean_shift.hip).  No ratio is promised or asserted.  Needs a GPU.
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


def example_cloud(seed=0):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=(1500, 3))
    p[:, 2] += 10.0
    for c in range(3):
        o = rng.normal(size=3)
        p[c * 500:(c + 1) * 500] += 2.5 * o / np.linalg.norm(o)
    return np.ascontiguousarray(p, np.float32)


def old_route(L, capi, points_dev, n, seeds, radius, conv_tol, passes):
    """-> (ms per pass, mean ball population) of `passes` passes of: list search of the active seeds, host mean, convergence test"""
    r2 = np.float32(radius) * np.float32(radius)
    s = seeds.copy()
    active = np.arange(s.shape[0])
    ms, pops = [], []
    for _ in range(passes):
        if active.size == 0:
            break
        t0 = time.perf_counter()
        q = np.ascontiguousarray(s[active])
        qd = __import__("torch").from_numpy(q).cuda()      # the upload of the seeds is part of the route
        offs = np.zeros(q.shape[0] + 1, np.uint64)
        total = C.c_size_t(0)
        rc = L.cilhip_radius_search3f(0, points_dev.data_ptr(), n, qd.data_ptr(), q.shape[0], capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, None, None, 0, C.byref(total))
        idx = np.zeros(max(int(total.value), 1), np.uint32)
        rc = rc or L.cilhip_radius_search3f(0, points_dev.data_ptr(), n, qd.data_ptr(), q.shape[0], capi.MEM_DEVICE, C.c_float(r2), offs.ctypes.data, idx.ctypes.data, None,
                                            int(total.value), C.byref(total))
        if rc != capi.OK:
            raise SystemExit(f"cilhip_radius_search3f failed: {rc}")
        o = offs.astype(np.int64)
        cnt = np.diff(o)
        host = old_route.host_points
        sums = np.add.reduceat(host[idx[: o[-1]]].astype(np.float64), np.minimum(o[:-1], max(o[-1] - 1, 0)), axis=0) if o[-1] else np.zeros((q.shape[0], 3))
        with np.errstate(invalid="ignore", divide="ignore"):
            new = (sums / cnt[:, None]).astype(np.float32)
        new[cnt == 0] = np.nan
        moved = ((q - new) ** 2).sum(axis=1)
        s[active] = new
        active = active[~(moved < np.float32(conv_tol) ** 2) & (cnt > 0)]
        ms.append(1e3 * (time.perf_counter() - t0))
        pops.append(float(cnt.mean()))
    return (float(np.mean(ms)) if ms else 0.0), (float(np.mean(pops)) if pops else 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--old-passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mean_shift_bench.json"))
    ap.add_argument("--cases", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/mean_shift_bench.py needs a GPU: there is no CPU path to time")
    from cilantro_amd import capi, clustering as cl
    from cilantro_amd import grid_downsampler as gd
    from components_bench import surface

    L = capi.load()
    dev = torch.device("cuda:0")
    f = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
    ds = gd.grid_downsample(torch.from_numpy(f["p1"]).to(dev), 0.005)["points"].cpu().numpy()
    surf = surface(1_000_000)[0]
    pick = np.random.default_rng(1).permutation(surf.shape[0])[:10_000]
    cases = [("example_3x500", example_cloud(), None, 2.0, 5000, 0.2, 1e-7), ("frame_1_downsampled", ds, None, 0.02, args.max_iter, 0.002, 1e-6),
             ("surface_1m_10k_seeds", surf, np.ascontiguousarray(surf[pick]), 0.02, args.max_iter, 0.002, 1e-6)]
    only = [c for c in args.cases.split(",") if c]
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "cases": {}}
    for name, p, seeds, radius, max_iter, tol, conv in cases:
        if only and name not in only:
            continue
        tp = torch.from_numpy(p).to(dev)
        ts = None if seeds is None else torch.from_numpy(seeds).to(dev)
        row = {"points": int(p.shape[0]), "seeds": int(p.shape[0] if seeds is None else seeds.shape[0]), "radius": radius, "max_iter": max_iter, "cluster_tol": tol,
               "convergence_tol": conv}
        for form in (1, 2, 0):
            best = None
            for rep in range(args.reps + 1):      # (the first call is the warm-up)
                t0 = time.perf_counter()
                r = cl.mean_shift(tp, radius, max_iter, tol, conv, seeds=ts, form=form)
                ms = 1e3 * (time.perf_counter() - t0)
                if rep and (best is None or ms < best[0]):
                    best = (ms, r)
            ms, r = best
            st = r["stats"]
            row[f"form_{form}"] = {"total_ms": ms, "shift_ms": st["shift_ms"], "ms_per_pass": st["shift_ms"] / max(st["passes"], 1), "passes": st["passes"], "iterations": r["iterations"],
                                   "group_ms": st["group_ms"], "rounds": st["rounds"], "clusters": int(r["offsets"].shape[0] - 1), "form_used": st["form_used"],
                                   "est_ball": st["est_ball"]}
        row["wave_over_lane"] = row["form_2"]["ms_per_pass"] / row["form_1"]["ms_per_pass"]
        old_route.host_points = p
        old_ms, pop = old_route(L, capi, tp, p.shape[0], p if seeds is None else seeds, radius, conv, args.old_passes)
        row["lists_and_host_mean"] = {"ms_per_pass": old_ms, "passes_timed": args.old_passes, "mean_ball_population": pop}
        result["cases"][name] = row
        print(f"{name:24s} {row['points']:8d} points {row['seeds']:6d} seeds, ball ~{pop:.0f} (estimated {row['form_0']['est_ball']:.0f}): per pass lane {row['form_1']['ms_per_pass']:.3f} ms, "
              f"wave {row['form_2']['ms_per_pass']:.3f} ms (x{row['wave_over_lane']:.2f}), picked form {row['form_0']['form_used']}; {row['form_0']['passes']} passes, total "
              f"{row['form_0']['total_ms']:.2f} ms; grouping {row['form_0']['group_ms']:.2f} ms in {row['form_0']['rounds']} rounds -> {row['form_0']['clusters']} clusters; "
              f"lists + host mean {old_ms:.2f} ms per pass", flush=True)
        del tp, ts
        torch.cuda.empty_cache()

    # what one pass's readback costs at least: a 4-byte device-to-host copy with its synchronisation, 200 times
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(20):
        word.item()
    t0 = time.perf_counter()
    for _ in range(200):
        word.item()
    result["readback_4_bytes_us"] = 1e6 * (time.perf_counter() - t0) / 200
    print(f"a 4-byte readback with its synchronisation: {result['readback_4_bytes_us']:.1f} us", flush=True)

    # the crossover of the two forms: frame_1 downsampled as its own seeds, five passes per radius
    if not only or "crossover" in only:
        tp = torch.from_numpy(ds).to(dev)
        sweep = []
        for radius in (0.01, 0.015, 0.02, 0.03, 0.04, 0.06, 0.08, 0.12):
            per = {}
            for form in (1, 2):
                cl.mean_shift(tp, radius, 5, 0.002, 0.0, form=form)
                st = min((cl.mean_shift(tp, radius, 5, 0.002, 0.0, form=form)["stats"] for _ in range(args.reps)), key=lambda s: s["shift_ms"])
                per[form] = st["shift_ms"] / max(st["passes"], 1)
            sweep.append({"radius": radius, "est_ball": st["est_ball"], "lane_ms_per_pass": per[1], "wave_ms_per_pass": per[2], "wave_over_lane": per[2] / per[1]})
            print(f"crossover: radius {radius:.3f} est. ball {st['est_ball']:8.1f}: lane {per[1]:.3f} ms, wave {per[2]:.3f} ms per pass (x{per[2] / per[1]:.2f})", flush=True)
        result["crossover_sweep_frame_1"] = sweep

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    main()
