#!/usr/bin/env python3
"""fgmres_multi (aggmg_fgmres_multi_dev) against K calls of fgmres on the same columns, on the config 3 / 4 hierarchy
(DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1), restart 30, tol 1e-8, zero guesses:

    python tools/exp_fgmres_multi.py --log2-elems 20 [--smoother blockJac|patchGS0] [--cycles 3,3 2,1] [--K 2 4 8]
                                     [--reps 10] [--no-split]

One process per size and smoother: run each under a time limit of its own.  patchGS0 switches AGGMG_OPT_PATCH_MULTI on.
Column 0 is the hierarchy's right-hand side, the others are standard normal.  Both sides run in the same process on the
same device buffers: wall time around the (synchronous) call, 3 warm-ups, then --reps runs of the one side and --reps
runs of the other -- not alternately, because the two solvers share the context's work space and an alternation would
time its exchange.  Per (cycle, K) one JSON line: medians, min and max of both sides, the ratio per column, the
iteration counts (asserted equal on both sides), the spread (max - min) of the K single calls and the verdict
`multi <= single + 3 x spread`.

split: the parts of ONE iteration at j = 0, 10, 29 on K columns, each timed alone around a synchronisation: the K-column
cycle, the K-column operator product, the orthogonalisation (the dots and the update + norms at nvec = j + 1, through
the stand-alone entries, which each read their scalars back), and a read-back of K (j + 2) doubles from an idle stream;
beside each the K single-vector calls it replaces."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=20)
    ap.add_argument("--smoother", default="blockJac", choices=["blockJac", "patchGS0"])
    ap.add_argument("--cycles", nargs="+", default=["3,3", "2,1"])
    ap.add_argument("--K", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxiter", type=int, default=200)
    ap.add_argument("--no-split", action="store_true")
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib, api, uniform
    ctx = mg.Context(0)
    lib, h = ctx.lib, ctx.handle
    if args.smoother == "patchGS0":
        ctx.set_option(_lib.OPT_PATCH_MULTI, 1)
    E = args.log2_elems
    U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
    H = uniform.build_device_hierarchy(U, ctx, smoother=args.smoother)
    op = H._ops[0]
    N = op.shape[0]
    Kmax = max(args.K)
    rng = np.random.default_rng(E)
    dB, dX, dZero = (mg.DeviceMatrix(ctx, N, Kmax) for _ in range(3))     # (fresh memory is zeroed)
    for j in range(Kmax):        # (column by column: no N x Kmax host matrix)
        col = U.rhs() if j == 0 else rng.standard_normal(N)
        ctx.check(lib.aggmg_memcpy_h2d(h, ctypes.c_void_p(dB.ptr.value + 8 * j * N), col.ctypes.data, 8 * N))
    pd, pi = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)

    def col(M, j):
        return ctypes.c_void_p(M.ptr.value + 8 * j * N)

    def wall(fn, before=None, reps=None, warm=3):
        """[ms] of fn() around a synchronisation, `before` untimed in front of every run"""
        ms = []
        for r in range(-warm, reps or args.reps):
            if before:
                before()
            ctx.synchronize()
            t0 = time.perf_counter()
            fn()
            ctx.synchronize()
            if r >= 0:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def stats(ms):
        return {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}

    for cyc in args.cycles:
        nPre, nPost = (int(v) for v in cyc.split(","))
        for K in args.K:
            hist = np.zeros(args.maxiter)
            it = ctypes.c_int(0)
            its_single = [0] * K
            out = {}

            def reset():
                api._copy_dev(ctx, dX.ptr.value, dZero.ptr.value, N * K)

            def singles():
                for j in range(K):
                    ctx.check(lib.aggmg_fgmres_dev(h, H.handle, col(dB, j), col(dX, j), args.restart, args.maxiter, args.tol,
                                                   nPre, nPost, 2.0 / 3.0, hist.ctypes.data_as(pd), ctypes.byref(it)))
                    its_single[j] = it.value

            def multi():
                out["multi"] = H.fgmres_multi_dev(dB, dX, K, N, args.restart, args.maxiter, args.tol, nPre, nPost)

            ts = wall(singles, reset)
            tm = wall(multi, reset)
            its, _, work = out["multi"]
            assert list(its) == its_single, (list(its), its_single)
            s, m = stats(ts), stats(tm)
            spread = s["max"] - s["min"]
            print(json.dumps({"what": "solve", "log2_elems": E, "N": N, "smoother": args.smoother, "cycle": f"V({nPre},{nPost})",
                              "K": K, "restart": args.restart, "tol": args.tol, "iterations": its_single, "work_cols": work,
                              "single_ms": s, "multi_ms": m, "ms_per_col_single": round(s["median"] / K, 4),
                              "ms_per_col_multi": round(m["median"] / K, 4), "ratio": round(m["median"] / s["median"], 4),
                              "spread_single_ms": round(spread, 4), "spread_single_rel": round(spread / s["median"], 4),
                              "no_slower_by_3_spreads": bool(m["median"] <= s["median"] + 3 * spread)}), flush=True)

    if not args.no_split:
        # the parts of one iteration; the basis is zeros (the time of a fused multiply-add does not depend on the values)
        nb = 30
        dV = ctx.alloc(nb * Kmax * N)
        dW, dZ = mg.DeviceMatrix(ctx, N, Kmax), mg.DeviceMatrix(ctx, N, Kmax)
        dW.upload(np.asfortranarray(rng.standard_normal((N, Kmax))))
        back = np.zeros(Kmax * (nb + 2))
        for cyc in args.cycles:
            nPre, nPost = (int(v) for v in cyc.split(","))
            for K in args.K:
                bs = N * K
                med = lambda fn: round(float(np.median(wall(fn, reps=max(5, args.reps // 2), warm=2))), 4)
                row = {"what": "split", "log2_elems": E, "smoother": args.smoother, "cycle": f"V({nPre},{nPost})", "K": K,
                       "cycle_multi_ms": med(lambda: H.vcycle_multi_dev(None, dW, dZ, K, N, nPre, nPost)),
                       "cycle_singles_ms": med(lambda: [ctx.check(lib.aggmg_vcycle_dev(h, H.handle, None, col(dW, j), nPre, nPost,
                                                                                      2.0 / 3.0, col(dZ, j))) for j in range(K)]),
                       "product_multi_ms": med(lambda: op.residual_multi_dev(dZ, None, dX, K, N)),
                       "product_singles_ms": med(lambda: [ctx.check(lib.aggmg_residual_dev(h, op.handle, col(dZ, j), col(dZero, j),
                                                                                          col(dX, j))) for j in range(K)])}
                for j in (0, 10, 29):
                    nvec = j + 1
                    c = np.full((K, nvec), 1e-9)

                    def ortho_multi():
                        ctx.multi_dot_cols(dV, dW, N, nvec, K, bstride=bs, cstride=N, ldw=N)
                        ctx.multi_axpy_norm_cols(dV, c, dW, N, nvec, K, bstride=bs, cstride=N, ldw=N)

                    def ortho_singles():
                        for k in range(K):
                            v = dV.ptr.value + 8 * k * N
                            ctx.multi_dot(v, col(dW, k).value, n=N, nvec=nvec, ld=bs)
                            ctx.multi_axpy_norm(v, c[k], col(dW, k).value, n=N, nvec=nvec, ld=bs)

                    def read_back():
                        ctx.check(lib.aggmg_memcpy_d2h(h, back.ctypes.data, dV.ptr, 8 * K * (j + 2)))

                    row[f"j={j}"] = {"ortho_multi_ms": med(ortho_multi), "ortho_singles_ms": med(ortho_singles),
                                     "read_back_ms": med(read_back)}
                print(json.dumps(row), flush=True)
        for v in (dV, dW, dZ):
            v.free()
    for v in (dB, dX, dZero):
        v.free()
    H.free()
    ctx.close()


if __name__ == "__main__":
    main()
