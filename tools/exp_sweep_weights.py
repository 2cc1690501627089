"""Sweep-weight schedules on the benchmark hierarchies: what a cycle costs and how many the solvers need, without a
schedule (alpha = 2/3 on every sweep) and with MeshHierarchy.set_chebyshev_smoothing() -- config 3 (DG p=3 -> AggDG 4:1 ->
2:1 -> 2:1) and config 5's shape (CG p=4 -> 2 -> 1 -> DG p=0), V(3,3), one GPU:

  * milliseconds per cycle of vcycles_dev, both ways (the weights ride in the kernel arguments of the same launches: the
    figures should be equal);
  * cycles and wall time of multigrid, iterations and wall time of pcg, to ||A x - b|| < tol ||b||, both ways, with the
    residual histories.

    python tools/exp_sweep_weights.py [--log2-elems 24] [--cg-log2-elems 24] [--levels 0] [--ratio 10] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def measure(mg, H, ctx, rhs, args, label):
    import numpy as np
    N = len(rhs)
    b, x0, y = ctx.to_device(rhs), ctx.to_device(np.zeros(N)), ctx.alloc(N)
    levels = [int(k) for k in args.levels.split(",")]

    def ms_per_cycle():
        H.vcycles_dev(x0, b, y, 3)                       # warm-up (lazy allocations, code objects)
        ctx.synchronize()
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            H.vcycles_dev(x0, b, y, args.cycles)
            ctx.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / args.cycles)
        return {"median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts))}

    def solve():
        out = {}
        ctx.synchronize()
        t0 = time.perf_counter()
        x, ncyc, res = mg.multigrid_dev(H, x0, b, args.maxiter, args.tol, check_every=1)
        ctx.synchronize()
        out["multigrid"] = {"cycles": ncyc, "ms": 1e3 * (time.perf_counter() - t0), "converged": bool(res and res[-1] < args.tol * nb),
                            "res_over_b": [r / nb for r in res]}
        x.free()
        t0 = time.perf_counter()
        _, it, resp = mg.pcg(H, rhs, maxiter=args.maxiter, tol=args.tol)
        out["pcg"] = {"iterations": it, "ms_with_host_transfers": 1e3 * (time.perf_counter() - t0),
                      "converged": bool(resp and resp[-1] < args.tol * nb), "res_over_b": [r / nb for r in resp]}
        return out

    nb = float(np.linalg.norm(rhs))
    r = {"workload": label, "unknowns": N, "tol": args.tol}
    H.clear_sweep_weights()
    r["unscheduled"] = {"ms_per_cycle": ms_per_cycle(), **solve()}
    t0 = time.perf_counter()
    lams = H.set_chebyshev_smoothing(levels=levels, ratio=args.ratio)
    r["chebyshev"] = {"levels": levels, "ratio": args.ratio, "lambda_max": lams, "setup_ms": 1e3 * (time.perf_counter() - t0),
                      "weights": {k: H.sweep_weights(k)[0].tolist() for k in levels}}
    r["chebyshev"].update({"ms_per_cycle": ms_per_cycle(), **solve()})
    H.clear_sweep_weights()
    # the unscheduled cycle once more: the spread of the figure within this process
    r["unscheduled_again_ms_per_cycle"] = ms_per_cycle()
    for v in (b, x0, y):
        v.free()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=24, help="config 3 size; 0 = skip")
    ap.add_argument("--cg-log2-elems", type=int, default=24, help="config 5 shape size; 0 = skip")
    ap.add_argument("--levels", default="0", help="comma-separated levels that get the Chebyshev schedule")
    ap.add_argument("--ratio", type=float, default=10.0)
    ap.add_argument("--cycles", type=int, default=10, help="cycles per timed vcycles_dev call")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--maxiter", type=int, default=150)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import uniform as U_
    ctx = mg.default_context()
    out = []
    if args.log2_elems:
        U = U_.UniformDgAggHierarchy(2 ** args.log2_elems, p=3, pAgg=1, ratios=(4, 2, 2))
        H = U_.build_device_hierarchy(U, ctx)
        out.append(measure(mg, H, ctx, U.rhs(), args, f"config 3: DG p=3 n=2^{args.log2_elems} -> AggDG 4:1 -> 2:1 -> 2:1, V(3,3)"))
        print(json.dumps(out[-1]), flush=True)
        H.free()
        del H, U
    if args.cg_log2_elems:
        U = U_.UniformCgDgHierarchy(2 ** args.cg_log2_elems, ps=(4, 2, 1))
        H = U_.build_device_cg_hierarchy(U, ctx)
        out.append(measure(mg, H, ctx, U.rhs(), args, f"config 5 shape: CG n=2^{args.cg_log2_elems} p=4 -> 2 -> 1 -> DG p=0, point Jacobi, V(3,3)"))
        print(json.dumps(out[-1]), flush=True)
        H.free()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
