#!/usr/bin/env python
"""Times the non-rigid ICP step on a sparse warp field (cilhip_warp_field_* through cilantro_amd.icp.WarpField)
beside the only route that existed before it, in the same run: lists and correspondences on the host, the scipy assembly of
tests/_warp_refs.py in f32, the explicit At At^T product, CG on the product.

    python tools/warp_field_bench.py [--reps 3] [--out profiles/warp_field_bench.json] [--cases frame_1,surface_1m] [--transform rigid|affine]

Cases: frame_1 (tests/golden/frames_full.npz p1 with its normals) after gridDownsample(0.005), against a bent copy of itself, control
nodes from gridDownsample(0.025) of the source, k = 4 / 8, the example's parameters (examples/non_rigid_icp.cpp:41-82); a 1M-point
synthetic surface against a bent 1M-point sample of it with about 10k control nodes.  Per case, whole-call wall times with the stream
drained (minimum of --reps after one warm-up):
  search            the context's set_source + find_correspondences + get_nn on the source (what an ICP iteration pays before the estimate)
  linearise         one estimate with max_gn_iter = 1, max_cg_iter = 0: match count, rows, arcs, A^T b and the diagonal, CG set-up, transforms out
  cg_iteration      (estimate with 16 CG iterations - estimate with 8) / 8, cg_conv_tol = 0 so that none stops early
  estimate          one estimate with the example's parameters (500 CG iterations at most, tolerance 1e-5) and its iteration count
and for the host route, once: assembly, product, one CG iteration (a sparse matrix-vector product and the vector updates), the whole
solve.  For one CG iteration the bytes it must move (the rows twice, the lists twice, u written and read, both transposed lists, the arcs'
derivatives twice, four vectors of 6 n_ctrl) and the fraction of the 6.29 TB/s a float4 copy reaches on this part are given -- at the
example's size the working set lies in L2 and the iteration is three dependent launches, so that fraction says nothing about the kernels
there and the JSON says so.  No ratio is promised or asserted.  Needs a GPU.

--transform affine times the same quantities for the affine entries (12 unknowns per node, a 12-float record per
source point) beside the scipy route of tests/_warp_affine_refs.py, with w_reg = 1 and at most 1000 CG iterations (at the example's
w_reg = 200 the affine system does not meet 1e-5 within the example's 500 iterations in f32), and writes them under the key "affine" of
the same JSON file, leaving the rigid rows as they are."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_MEASURED = 6.29e12


def best(fn, reps):
    fn()
    out = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        out = min(out, 1e3 * (time.perf_counter() - t0))
    return out, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_field_bench.json"))
    ap.add_argument("--cases", default="frame_1,surface_1m")
    ap.add_argument("--host-route-max-points", type=int, default=200000, help="the scipy route is skipped above this many source points")
    ap.add_argument("--transform", choices=("rigid", "affine"), default="rigid")
    a = ap.parse_args()
    affine = a.transform == "affine"
    nu = 12 if affine else 6
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("tools/warp_field_bench.py needs a GPU: there is no CPU path to time")
    import _warp_affine_refs as WA
    import _warp_refs as W
    from cilantro_amd import capi, grid_downsampler as gd, synthetic
    from cilantro_amd.icp import Context, WarpField, RBFKernelWeightEvaluator
    from cilantro_amd.normal_estimation import KDTree3f
    from components_bench import surface

    cases = {}
    if "frame_1" in a.cases:
        f = np.load(os.path.join(ROOT, "tests", "golden", "frames_full.npz"))
        ds = gd.grid_downsample(f["p1"], 0.005, normals=f["n1"])
        src = np.ascontiguousarray(ds["points"], np.float32)
        ext = float((src.max(0) - src.min(0)).max())
        cases["frame_1_downsampled"] = dict(src=src, dst=synthetic.bend(src - src.min(0), 0.004, ext) + src.min(0), dst_n=np.ascontiguousarray(ds["normals"], np.float32), res=0.025,
                                            max_sq=0.02 ** 2)
    if "surface_1m" in a.cases:
        src, _ = surface(1_000_000, seed=45)
        flat, nrm = surface(1_000_000, seed=46)
        cases["surface_1m"] = dict(src=src, dst=synthetic.bend(flat, 0.004), dst_n=nrm, res=0.0105, max_sq=0.02 ** 2)

    doc = {"tool": "tools/warp_field_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "hbm_reference_bytes_per_s": HBM_MEASURED, "results": {}}
    for name, c in cases.items():
        src, dst, dst_n, res = c["src"], c["dst"], c["dst_n"], c["res"]
        ctrl = np.ascontiguousarray(gd.grid_downsample(src, res)["points"], np.float32)
        tree = KDTree3f(ctrl)
        s2c, reg = tree.kNNSearch(src, 4), tree.kNNSearch(ctrl, 8)
        n_src, n_ctrl = len(src), len(ctrl)
        ce, re = RBFKernelWeightEvaluator(0.5 * res), RBFKernelWeightEvaluator(3.0 * res)
        t0 = time.perf_counter()
        wf = WarpField(n_src, n_ctrl, s2c, ce, reg, re)
        create_ms = 1e3 * (time.perf_counter() - t0)
        ctx = Context(0)
        ctx.set_target(dst, dst_n)

        def search():
            ctx.set_source(src)
            ctx.find_correspondences(np.eye(4, dtype=np.float32), c["max_sq"], count=False)
            return ctx.get_nn()[0]

        search_ms, nn = best(search, a.reps)

        def params(**kw):
            p = capi.WarpParams()
            capi.load().cilhip_warp_default_params(C.byref(p))
            base = dict(w_p2p=0.0, w_p2pl=1.0, w_reg=1.0 if affine else 200.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=1000 if affine else 500,
                        cg_conv_tol=1e-5)
            base.update(kw)
            for k, v in base.items():
                setattr(p, k, v)
            return p

        def est(p):
            return lambda: wf.estimate(dst, dst_n, src, nn, p, affine=affine)

        # (host arrays: every call also uploads the clouds -- measured alone, below, and reported beside the times)
        def upload():
            for x in (dst, dst_n, src):
                torch.from_numpy(x).cuda()
            torch.cuda.synchronize()

        upload_ms, _ = best(upload, a.reps)
        lin_ms, _ = best(est(params(max_cg_iter=0)), a.reps)
        cg8, _ = best(est(params(max_cg_iter=8, cg_conv_tol=0.0)), a.reps)
        cg16, _ = best(est(params(max_cg_iter=16, cg_conv_tol=0.0)), a.reps)
        est_ms, (_, st) = best(est(params()), a.reps)
        idx = np.asarray(s2c[0])
        valid, n_arcs = int((idx >= 0).sum()), int((np.asarray(reg[0])[:, 1:] >= 0).sum())
        matched = int((nn != capi.NONE_IDX).sum())
        # (the record is 96 B per point, 48 B with affine transforms; an arc's derivatives and u are 4 nu B each, a vector 4 nu n_ctrl B)
        cg_bytes = 2 * (48 if affine else 96) * matched + 2 * 8 * valid + 2 * 16 * n_src + 4 * valid + 2 * 4 * nu * n_arcs + 2 * 4 * nu * n_arcs + 8 * n_arcs + 8 * n_arcs + 4 * 4 * nu * n_ctrl
        cg_ms = (cg16 - cg8) / 8.0
        row = {"source_points": n_src, "target_points": len(dst), "control_nodes": n_ctrl, "arcs": n_arcs, "matches": matched, "create_ms": create_ms, "search_ms": search_ms,
               "upload_of_the_three_clouds_ms": upload_ms, "linearise_ms": lin_ms, "cg_iteration_ms": cg_ms, "estimate_ms": est_ms, "estimate_cg_iterations": int(st.cg_iterations_total),
               "estimate_converged": int(st.converged), "cg_iteration_bytes": cg_bytes, "cg_iteration_fraction_of_hbm_reference": cg_bytes / (cg_ms * 1e-3) / HBM_MEASURED if cg_ms > 0 else None,
               "cg_iteration_note": "three dependent launches per iteration; where cg_iteration_bytes is below the 32 MiB of L2 the iteration is launch-bound and the HBM fraction says nothing about the kernels"}
        if n_src <= a.host_route_max_points:
            g = W.Graph(n_ctrl, np.where(idx < 0, W.NONE, idx).astype(np.uint32), s2c[1], W.RBF, 0.5 * res, np.where(np.asarray(reg[0]) < 0, W.NONE, reg[0]).astype(np.uint32), reg[1], W.RBF,
                        3.0 * res)
            p = W.Params(w_p2p=0.0, w_p2pl=1.0, w_reg=1.0 if affine else 200.0, huber_boundary=1e-2, max_gn_iter=1, gn_conv_tol=5e-4, max_cg_iter=1000 if affine else 500, cg_conv_tol=1e-5)
            t0 = time.perf_counter()
            if affine:
                At, b, _ = WA.assemble(g, np.float32, dst, dst_n, src, nn, WA.identity_start(n_ctrl, np.float32), p, sort=True)
            else:
                At, b, _ = W.assemble(g, np.float32, dst, dst_n, src, nn, np.zeros(6 * n_ctrl, np.float32), p, sort=True)
            t1 = time.perf_counter()
            AtA = (At @ At.T).tocsc()
            Atb = At @ b
            t2 = time.perf_counter()
            x, its, _ = W.eigen_cg(AtA, Atb, p.cg_conv_tol, p.max_cg_iter, np.float32)
            t3 = time.perf_counter()
            row["host_route_ms"] = {"assemble": 1e3 * (t1 - t0), "product": 1e3 * (t2 - t1), "cg": 1e3 * (t3 - t2), "cg_iterations": int(its),
                                    "cg_iteration": 1e3 * (t3 - t2) / max(int(its), 1), "total": 1e3 * (t3 - t0)}
        else:
            row["host_route_ms"] = None
        doc["results"][name] = row
        print(name, json.dumps(row), flush=True)
        wf.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if affine:      # the rigid rows stay as they are: the affine ones go under a key of their own
        kept = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                kept = json.load(fh)
        kept["affine"] = {k: doc[k] for k in ("device", "reps", "results")}
        doc = kept
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
