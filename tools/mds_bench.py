#!/usr/bin/env python
"""Times multidimensional scaling (cilhip_mds_embedding / cilhip_mds_apply through cilantro_amd.multidimensional_scaling).

    python tools/mds_bench.py [--reps 3] [--out profiles/mds_bench.json] [--sizes 1000,8192,32768] [--scipy-max-points 8192]

Cases: the example's wobbling circle (1000 points) and Gaussian clouds in 5-D with scales (5, 3, 2, 1, 0.5) at the larger sizes; the squared
distances are formed on the device and stay there (n = 32768: a 4.3 GB matrix).  Per case:
  block_product   one product Y = B X of the operator that is never formed, by device events around the product alone (cilhip_mds_apply;
                  minimum of --reps after one warm-up), at the example's block width 5 and at the widest block, 25: the matrix bytes (4 n^2)
                  over that time as a fraction of the float4 copy rate measured in the same run, all bytes (with the chunk partial sums
                  written and read back and the blocks), and the f64 FLOP rate (2 n^2 b)
  embedding       the whole call for 2 dimensions, wall time with the stream drained (minimum of --reps after one warm-up), with its outer
                  iterations, block products and largest residual
  numpy_scipy     the only route that existed before, timed in the same run up to --scipy-max-points: B formed with numpy in f64, then
                  scipy.sparse.linalg.eigsh(which="LM")
No ratio is promised or asserted.  Needs a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mds_bench.json"))
    ap.add_argument("--sizes", default="1000,8192,32768")
    ap.add_argument("--scipy-max-points", type=int, default=8192)
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/mds_bench.py needs a GPU: there is no CPU path to time")
    import _mds_refs as R
    from cilantro_amd import multidimensional_scaling as mds
    from spectral_bench import best, copy_rate

    rate = copy_rate(torch)
    doc = {"tool": "tools/mds_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "float4_copy_bytes_per_s": rate, "results": {}}
    for n in [int(v) for v in a.sizes.split(",")]:
        if n == 1000:
            name, D = "circle_1000", torch.from_numpy(R.circle(1000)[0]).cuda()
        else:
            name = "gauss5_%d" % n
            P = torch.from_numpy(np.random.default_rng(n).standard_normal((n, 5)) * np.array([5.0, 3.0, 2.0, 1.0, 0.5])).cuda()
            sq = (P * P).sum(1)
            D = (sq[:, None] + sq[None, :] - 2.0 * (P @ P.T)).clamp_(min=0.0)
            D = (0.5 * (D + D.T)).float().contiguous()
            D.fill_diagonal_(0.0)
            del P, sq
        torch.cuda.synchronize()
        chunks = (n + max(128, (n + 63) // 64) - 1) // max(128, (n + 63) // 64)
        row = {"points": n, "matrix_bytes": 4 * n * n, "chunks": chunks, "block_product": {}}
        for b in (5, 25):
            X = torch.from_numpy(np.random.default_rng(b).uniform(-1.0, 1.0, (n, b))).cuda()
            ms = min(mds.mds_apply(D, X)[1] for _ in range(a.reps + 1))
            all_bytes = 4 * n * n + 2 * chunks * n * b * 8 + 4 * n * b * 8
            row["block_product"]["b%d" % b] = {
                "ms": ms, "matrix_bytes_per_s": 4 * n * n / (ms * 1e-3), "matrix_fraction_of_copy_rate": 4 * n * n / (ms * 1e-3) / rate, "all_bytes": all_bytes,
                "all_bytes_fraction_of_copy_rate": all_bytes / (ms * 1e-3) / rate, "f64_tflops": 2.0 * n * n * b / (ms * 1e-3) / 1e12}
        emb_ms, (E, ev, info) = best(lambda: mds.mds_embedding(D, 2), a.reps)
        row["embedding_ms"] = emb_ms
        row["embedding"] = {key: (float(v) if isinstance(v, float) else int(v)) for key, v in info.items()}
        row["eigenvalues"] = [float(v) for v in ev]
        row["numpy_scipy_ms"] = None
        if n <= a.scipy_max_points:
            try:
                from scipy.sparse.linalg import eigsh

                Dh = D.cpu().numpy()
                t0 = time.perf_counter()
                B = R.centred(Dh)
                t1 = time.perf_counter()
                w = eigsh(B, k=2, which="LM", tol=1e-7, ncv=4, maxiter=100000, return_eigenvectors=True)[0]
                row["numpy_form_B_ms"] = 1e3 * (t1 - t0)
                row["numpy_scipy_ms"] = 1e3 * (time.perf_counter() - t0)
                row["numpy_scipy_eigenvalues"] = [float(v) for v in sorted(w, key=lambda v: -abs(v))]
                del B, Dh
            except ImportError:
                pass
            except Exception as e:      # (ARPACK may give up on a repeated eigenvalue: recorded, not hidden)
                row["numpy_scipy_error"] = str(e)[:200]
        row["note"] = "a matrix below the 32 MiB of L2 / 256 MiB of Infinity Cache is not streamed from HBM: its fractions say nothing about the memory system"
        doc["results"][name] = row
        print(name, json.dumps(row), flush=True)
        del D
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
