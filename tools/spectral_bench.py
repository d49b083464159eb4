#!/usr/bin/env python
"""Times the spectral embedding (cilhip_spectral_embedding through cilantro_amd.clustering) and the steps around it.

    python tools/spectral_bench.py [--reps 3] [--out profiles/spectral_bench.json] [--cases shells,surface_1m]

Cases: the example's two shells (1700 points, 30 neighbours) and a 1M-point synthetic surface (10 neighbours), both with the RBF kernel
and forced symmetry.  Per case, whole-call wall times with the stream drained (minimum of --reps after one warm-up):
  knn, graph        cilhip_knn3f and cilhip_nn_graph_matrix on host arrays
  block_product     (embedding with max_outer = 2 and a filter of degree 64 - the same with degree 32) / 32: one step Y = alpha (A X - c X) + beta Z
                    of the filter's recurrence, with the bytes it must move -- the matrix once (columns, values, the gathered scale), the
                    three blocks once -- and, separately, the bytes of the gathered rows of X, which come out of the caches when the matrix
                    is banded; both against the float4 copy rate measured in the same run
  embedding         the whole call with the reference's settings (at most 4 clusters, estimated, random walk), its outer iterations, block
                    products, converged pairs and largest residual.  A connected surface of a million points has its lowest eigenvalues
                    within 1e-5 of each other: the filter separates them by a factor near 1.005 per outer iteration, so above 100 000
                    points the call is limited to --max-outer iterations and the row says how far it got (n_converged, max_residual)
  kmeans            cilhip_kmeans_nd on the embedding
and, where scipy is installed and the case has at most --scipy-max-points points, scipy.sparse.linalg.eigsh on the same matrix beside it.
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


def best(fn, reps):
    fn()
    out, r = float("inf"), None
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out = min(out, 1e3 * (time.perf_counter() - t0))
    return out, r


def copy_rate(torch):
    """bytes per second of a float4-wide device copy (read + write), 1 GiB"""
    src = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    best_s = float("inf")
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        best_s = min(best_s, time.perf_counter() - t0)
    return 2.0 * src.numel() * 4 / best_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectral_bench.json"))
    ap.add_argument("--cases", default="shells,surface_1m")
    ap.add_argument("--scipy-max-points", type=int, default=200000)
    ap.add_argument("--max-outer", type=int, default=40, help="outer iterations the embedding of a case above 100 000 points may take")
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/spectral_bench.py needs a GPU: there is no CPU path to time")
    import _spectral_refs as R
    from cilantro_amd import clustering as cl
    from cilantro_amd.normal_estimation import KDTree3f

    cases = {}
    if "shells" in a.cases:
        cases["shells_1700"] = (R.cloud("shells")[0], 30)
    if "surface_1m" in a.cases:
        from components_bench import surface

        cases["surface_1m"] = (surface(1_000_000, seed=45)[0], 10)
    rate = copy_rate(torch)
    doc = {"tool": "tools/spectral_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "float4_copy_bytes_per_s": rate, "results": {}}
    for name, (P, k) in cases.items():
        P = np.ascontiguousarray(P, np.float32)
        knn_ms, (idx, d2, _) = best(lambda: KDTree3f(P).kNNSearch(None, k), a.reps)
        ev = cl.RBFKernelWeightEvaluator(1.0)

        def build():
            W = cl.nn_graph_sparse_matrix((idx, d2), ev, True)
            W.close()

        graph_ms, _ = best(build, a.reps)
        W = cl.nn_graph_sparse_matrix((idx, d2), ev, True)
        n, nnz, longest = W.info()

        def filtered(degree):      # (two outer iterations do not converge: the call still returns CILHIP_OK)
            return lambda: cl.spectral_embedding(W, 4, True, max_outer=2, degree=degree, raise_unconverged=False)

        t32, _ = best(filtered(32), a.reps)
        t64, _ = best(filtered(64), a.reps)
        product_ms = (t64 - t32) / 32.0
        b = 5 + 3      # nev = 5, guard 3
        stream_bytes = nnz * (4 + 4) + n * (8 + 8 + 8 + 8) + 3 * n * b * 8
        gather_bytes = nnz * (b * 8 + 8)
        limit = a.max_outer if n > 100000 else None
        emb_ms, (E, lam, info) = best(lambda: cl.spectral_embedding(W, 4, True, max_outer=limit, raise_unconverged=False), a.reps)
        km_ms, km = best(lambda: cl.KMeansXf(E).cluster(E.shape[1], seed=0), a.reps)
        row = {"points": n, "neighbours": k, "nnz": nnz, "longest_row": longest, "knn_ms": knn_ms, "graph_ms": graph_ms, "block_columns": b, "block_product_ms": product_ms,
               "block_product_stream_bytes": stream_bytes, "block_product_gather_bytes": gather_bytes,
               "block_product_stream_fraction_of_copy_rate": stream_bytes / (product_ms * 1e-3) / rate if product_ms > 0 else None,
               "block_product_stream_plus_gather_fraction_of_copy_rate": (stream_bytes + gather_bytes) / (product_ms * 1e-3) / rate if product_ms > 0 else None,
               "embedding_ms": emb_ms, "embedding_max_outer": limit if limit is not None else 1000,
               "embedding": {key: (float(v) if isinstance(v, float) else int(v)) for key, v in info.items()}, "eigenvalues": [float(v) for v in lam],
               "kmeans_ms": km_ms, "kmeans_iterations": km.getNumberOfPerformedIterations(),
               "note": "where stream + gather bytes are below the 32 MiB of L2 a block product is launch-bound and the fractions say nothing about the kernel"}
        row["scipy_eigsh_ms"] = None
        if n <= a.scipy_max_points:
            try:
                import scipy.sparse as sp
                from scipy.sparse.linalg import eigsh

                off, col, val = W.get()
                Ws = sp.csr_matrix((val.astype(np.float64), col.astype(np.int64), off.astype(np.int64)), (n, n))
                s = 1.0 / np.sqrt(np.asarray(Ws.sum(1)).ravel())
                A = (sp.identity(n) - sp.diags(s) @ Ws @ sp.diags(s)).tocsr()
                t0 = time.perf_counter()
                w = eigsh(A, k=5, which="SA", tol=1e-7, ncv=10, maxiter=100000, return_eigenvectors=True)[0]
                row["scipy_eigsh_ms"] = 1e3 * (time.perf_counter() - t0)
                row["scipy_eigsh_eigenvalues"] = [float(v) for v in np.sort(w)]
            except ImportError:
                pass
            except Exception as e:      # (ARPACK may give up on a repeated eigenvalue: recorded, not hidden)
                row["scipy_eigsh_error"] = str(e)[:200]
        doc["results"][name] = row
        print(name, json.dumps(row), flush=True)
        W.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
