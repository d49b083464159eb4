#!/usr/bin/env python
"""Times the voxel-grid downsampler (cilhip_grid_downsample3f through cilantro_amd.grid_downsampler) on device-resident clouds,
beside the yardstick of the same run: the target index build (csrc/grid_build.hip -- key, stable sort, segment table, gather: the
same kind of work) on the same 10M-point cloud.

    python tools/grid_downsample_bench.py [--n 10000000] [--reps 5] [--out profiles/grid_downsample_bench.json] [--cases a,b,...]

Per case: bins, milliseconds (device events around the call; minimum and median of --reps calls after two warm-up calls) and GB/s
against the bytes the algorithm must move, computed from the shapes: every input read once, every output written once, and the radix
sort's passes over (key, index).  `chain_bytes` is what the kernel chain as built moves on top of that (the range pass, the head
flags and scans, the gathered copy the folds read).  Needs a GPU: there is no CPU path to time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def key_bits(points, bin_size):
    """bits of the sort key the library packs: per axis the bits that hold (max cell - min cell) -> (bits, key bytes)"""
    inv = np.float32(1.0) / np.float32(bin_size)
    bits = 0
    for a in range(3):
        c = np.floor(points[:, a] * inv)
        bits += int(c.max() - c.min()).bit_length()
    return bits, (4 if bits + 1 <= 32 else 8)


def byte_model(n, bins, attrs, bits, key_bytes, lexicographic=True):
    """attrs: 12-byte attributes per point (points, + normals, + colours)"""
    passes = max(1, -(-max(bits, 1) // 8))      # 8 bits per pass of the LSD sort
    pair = key_bytes + 4
    sort = key_bytes * n + passes * 2 * pair * n      # one histogram read of the keys, then read + write of the pairs per pass
    must = 12 * attrs * n + (12 * attrs + 4) * bins + sort
    chain = must + 12 * n + (12 * n + pair * n) + (key_bytes + 4 + 8 + 4) * n + 4 * n + 2 * 12 * attrs * n + (0 if lexicographic else 12 * n)
    return {"must_bytes": int(must), "chain_bytes": int(chain), "sort_passes": passes, "key_bits": bits, "key_bytes": key_bytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grid_downsample_bench.json"))
    ap.add_argument("--cases", default="")
    args = ap.parse_args()

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/grid_downsample_bench.py needs a GPU: there is no CPU path to time")
    from cilantro_amd import grid_downsampler as gd
    from cilantro_amd import synthetic as syn
    from cilantro_amd.icp import Context

    n = args.n
    pts = syn.make_dst(n)
    nrm = syn.make_normals(n)
    col = syn.uniform01(45, 3 * n).reshape(n, 3)
    bin8 = float(np.float32((8.0 / n) ** (1.0 / 3.0)))      # unit cube, about 8 points per bin
    f = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
    one = (pts * np.float32(0.999)).astype(np.float32)      # every point in cell (0, 0, 0) of a unit grid
    cases = [
        ("synthetic_normals", pts, nrm, None, bin8, True),
        ("synthetic_normals_first_appearance", pts, nrm, None, bin8, False),
        ("synthetic_normals_colors", pts, nrm, col, bin8, True),
        ("synthetic_points_only", pts, None, None, bin8, True),
        ("frames_full_0.005", f["p1"], f["n1"], None, 0.005, True),
        ("one_bin_points", one, None, None, 1.0, True),
        ("one_bin_normals", one, nrm, None, 1.0, True),
    ]
    only = [c for c in args.cases.split(",") if c]
    dev = torch.device("cuda:0")
    result = {"device": torch.cuda.get_device_name(0), "n": n, "reps": args.reps, "cases": {}}

    def timed(fn):
        for _ in range(2):
            fn()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return float(min(ms)), float(np.median(ms))

    # the yardstick: the index build of the ICP target over the same cloud (device-resident input, as for the downsampler)
    tp, tn = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
    ctx = Context(0)
    built = []

    def build():
        ctx.set_target(tp, tn)
        ctx.synchronize()
        built.append(ctx.grid_info().build_ms)

    lo, med = timed(build)
    result["index_build_yardstick"] = {"points": n, "ms_min": lo, "ms_median": med, "library_build_ms_min": float(min(built[2:])),
                                       "what": "cilhip_set_target on device-resident points + normals: copy, cell keys, stable sort, cell table, gather"}
    print(f"yardstick: target index build, {n} points + normals: {lo:.2f} ms (median {med:.2f}; the library's own clock {min(built[2:]):.2f})", flush=True)
    ctx.close()
    del tp, tn

    for name, p, nn, cc, bin_size, lex in cases:
        if only and name not in only:
            continue
        p = np.ascontiguousarray(p, np.float32)
        t = [torch.from_numpy(p).to(dev), None if nn is None else torch.from_numpy(np.ascontiguousarray(nn[: p.shape[0]], np.float32)).to(dev),
             None if cc is None else torch.from_numpy(np.ascontiguousarray(cc, np.float32)).to(dev)]
        out = {}

        def call():
            out["r"] = gd.grid_downsample(t[0], bin_size, normals=t[1], colors=t[2], parallel=lex)

        lo, med = timed(call)
        bins = int(out["r"]["points"].shape[0])
        attrs = 1 + (nn is not None) + (cc is not None)
        bits, kb = key_bits(p, bin_size)
        model = byte_model(p.shape[0], bins, attrs, bits, kb, lex)
        row = {"points": int(p.shape[0]), "attributes": attrs, "bin_size": bin_size, "lexicographic": lex, "bins": bins, "points_per_bin": p.shape[0] / max(bins, 1),
               "ms_min": lo, "ms_median": med, "gbps_must": model["must_bytes"] / lo / 1e6, "gbps_chain": model["chain_bytes"] / lo / 1e6, **model,
               "over_index_build": lo / result["index_build_yardstick"]["ms_min"]}
        if bins == 1:
            row["ns_per_member"] = 1e6 * lo / p.shape[0]      # the whole call over the chain's length: an upper bound of the time per dependent add
        result["cases"][name] = row
        print(f"{name:40s} {p.shape[0]:9d} points -> {bins:8d} bins  {lo:8.2f} ms (median {med:.2f})  {row['gbps_must']:7.1f} GB/s of the bytes it must move "
              f"({model['must_bytes'] / 1e6:.0f} MB, {model['sort_passes']} sort passes over {kb}-byte keys)  x{row['over_index_build']:.2f} of the index build", flush=True)
        del t, out
        torch.cuda.empty_cache()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
