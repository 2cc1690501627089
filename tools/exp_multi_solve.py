#!/usr/bin/env python3
"""K right-hand sides through the outer loops (aggmg_pcg_multi_dev, aggmg_multigrid_multi_dev) against K single-vector
calls (aggmg_pcg_dev, aggmg_multigrid_dev in its default form), on the config 3/4 hierarchy (DG p = 3 -> AggDG 4:1 ->
2:1 -> 2:1):

    python tools/exp_multi_solve.py [--log2-elems 22 24] [--K 1 2 4 8] [--reps 7] [--iters 6]
    python tools/exp_multi_solve.py --profile-only K --log2-elems 22    # the command rocprofv3 runs (one K, no timing)

Both solvers run a fixed number of iterations (tol = 0: no column ever leaves, so K-column and single calls do the same
work per column), the K-column call and the K single calls timed alternately in one process after one warm-up call of
each, medians of --reps.  The K-column residual alone (aggmg_residual_multi_dev) and K single residuals are timed from
HIP events (profiling mode 1, kind `residual`); its compulsory bytes (aggmg_residual_multi_launch_bytes: operator arrays
once, vectors once per column) over that time give the fraction of 8 TB/s.  The alternating calls stream 1.3 GB (2^22)
of fine operator and several N x K matrices between two passes over the same operator: nothing of it survives in the
256 MB Infinity Cache.  One JSON line per (size, K)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, nargs="+", default=[22, 24])
    ap.add_argument("--K", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=6, help="pcg iterations / multigrid cycles per call")
    ap.add_argument("--profile-only", type=int, default=0, metavar="K",
                    help="run one warm-up and one K-column pcg and multigrid call and nothing else (for rocprofv3)")
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import uniform
    ctx = mg.Context(0)
    lib, h = ctx.lib, ctx.handle
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
    it = args.iters
    for E in args.log2_elems:
        U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
        H = uniform.build_device_hierarchy(U, ctx)
        op = H._ops[0]
        N = op.shape[0]
        Kmax = args.profile_only or max(args.K)
        rng = np.random.default_rng(E)
        dB, dX0, dX, dR = (mg.DeviceMatrix(ctx, N, Kmax) for _ in range(4))
        dB.upload(rng.standard_normal((N, Kmax)))
        xo = ctx.alloc(N)
        col = lambda M, j: ctypes.c_void_p(M.ptr.value + 8 * j * N)
        hist = np.zeros(max(it, 1))
        n1, n2 = ctypes.c_int(0), ctypes.c_int(0)

        def pcg_multi(K):
            H.pcg_multi_dev(dB, dX, K, N, maxiter=it, tol=0.0)

        def pcg_single(K):
            for j in range(K):
                ctx.check(lib.aggmg_pcg_dev(h, H.handle, col(dB, j), col(dX, j), it, 0.0, 3, 3, 2.0 / 3.0,
                                            hist.ctypes.data_as(pd), ctypes.byref(n1)))

        def mg_multi(K):
            H.multigrid_multi_dev(dX0, dB, dX, it, 0.0, K, N)

        def mg_single(K):
            for j in range(K):
                ctx.check(lib.aggmg_multigrid_dev(h, H.handle, col(dX0, j), col(dB, j), it, 0.0, 1, 3, 3, 2.0 / 3.0, xo.ptr,
                                                  hist.ctypes.data_as(pd), ctypes.byref(n1), ctypes.byref(n2), None, None))

        def res_multi(K):
            op.residual_multi_dev(dX0, dB, dR, K, N)

        def res_single(K):
            for j in range(K):
                ctx.check(lib.aggmg_residual_dev(h, op.handle, col(dX0, j), col(dB, j), xo.ptr))

        if args.profile_only:
            for _ in range(2):
                pcg_multi(Kmax)
                mg_multi(Kmax)
            ctx.synchronize()
            print(json.dumps({"log2_elems": E, "K": Kmax, "multi_info": H.multi_info(Kmax)}))
            H.free()
            continue

        def timed(fn, K):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn(K)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        def pair(fm, fs, K):
            fm(K)
            fs(K)
            tm, ts = [], []
            for _ in range(args.reps):   # alternating
                tm.append(timed(fm, K))
                ts.append(timed(fs, K))
            return float(np.median(tm)), float(np.median(ts))

        def events(fn, K):
            fn(K)
            ctx.synchronize()
            ctx.profile_enable(1)
            for _ in range(args.reps):
                fn(K)
            st = ctx.profile_collect()
            ctx.profile_enable(False)
            ms, n = st.get(("residual", 0), (0.0, 0))
            return ms / args.reps, n // args.reps   # ms of the residual launches of one call, their number

        for K in args.K:
            fused, group = H.multi_info(K)
            pm, ps = pair(pcg_multi, pcg_single, K)
            mm, ms = pair(mg_multi, mg_single, K)
            rm, nrm = events(res_multi, K)
            rs, nrs = events(res_single, K)
            rd, wr = 0, 0
            for c0 in range(0, K, group):
                r_, w_ = op.residual_multi_launch_bytes(min(group, K - c0))
                rd, wr = rd + r_, wr + w_
            r1, w1 = mg.smoother_launch_bytes(op, None, "residual")
            print(json.dumps({
                "log2_elems": E, "K": K, "fused": fused, "group": group, "iters": it,
                "pcg_ms_multi": round(pm, 3), "pcg_ms_single_xK": round(ps, 3), "pcg_per_col_ratio": round(pm / ps, 4),
                "mg_ms_multi": round(mm, 3), "mg_ms_single_xK": round(ms, 3), "mg_per_col_ratio": round(mm / ms, 4),
                "res_ms_multi": round(rm, 4), "res_launches_multi": nrm, "res_ms_single_xK": round(rs, 4),
                "res_launches_single": nrs, "res_per_col_ratio": round(rm / rs, 4) if rs > 0 else None,
                "res_bytes_multi": rd + wr, "res_frac_8TBs_multi": round((rd + wr) / (rm * 1e-3) / PEAK, 4) if rm > 0 else None,
                "res_bytes_single_xK": K * (r1 + w1),
                "res_frac_8TBs_single": round(K * (r1 + w1) / (rs * 1e-3) / PEAK, 4) if rs > 0 else None}), flush=True)
        for v in (dB, dX0, dX, dR, xo):
            v.free()
        H.free()


if __name__ == "__main__":
    main()
