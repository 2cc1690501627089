#!/usr/bin/env python3
"""Flexible GMRES around the V-cycle (aggmg_fgmres_dev) and the two streaming passes of its orthogonalisation, on the
config 3 hierarchy (DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1):

    python tools/exp_fgmres.py [--log2-elems 22 24] [--nvec 1 8 9 16 30] [--reps 20] [--no-solve]

Times are HIP events on the context's stream (a torch stream the context is given), 3 warm-up calls, medians of --reps.

passes: at every nvec the fused dots (aggmg_multi_dot_dev), the fused update with its norm (aggmg_multi_axpy_norm_dev)
and, in the same process, nvec calls of aggmg_dot_dev.  Bytes: per group of g <= 8 vectors the dots read (g + 1) 8N, the
update reads (g + 1) 8N and writes 8N; given as a fraction of 8 TB/s and of the 6.29 TB/s copy ceiling.

iteration: one V-cycle from a zero guess, one operator product (the residual launch), and the orthogonalisation at
nvec = j + 1 for j = 0, 10, 29 -- the three parts of iteration j of a restart cycle.

solve: time and iterations to 1e-8 ||b|| of multigrid V(3,3), pcg V(3,3), fgmres V(3,3), V(2,1), V(1,1); then the same
with a Chebyshev schedule on level 0 (degree = the sweep count of each half, the post half reversed).  One JSON line
per measurement."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK, COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, nargs="+", default=[22, 24])
    ap.add_argument("--nvec", type=int, nargs="+", default=[1, 8, 9, 16, 30])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--no-solve", action="store_true")
    args = ap.parse_args()
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import uniform
    ctx = mg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    lib, h = ctx.lib, ctx.handle

    def timed(fn, reps=None, warm=3):
        """median ms of fn() between two events on the context's stream"""
        for _ in range(warm):
            fn()
        ms = []
        for _ in range(reps or args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ctx.synchronize()
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms))

    for E in args.log2_elems:
        U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
        H = uniform.build_device_hierarchy(U, ctx)
        op = H._ops[0]
        N = op.shape[0]
        b = U.rhs()
        nb = float(np.linalg.norm(b))
        rng = np.random.default_rng(E)
        kmax = max(max(args.nvec), 30)
        dV = mg.DeviceMatrix(ctx, N, kmax)
        for j in range(kmax):        # (column by column: no N x kmax host matrix)
            col = rng.standard_normal(N) / np.sqrt(N)
            ctx.check(lib.aggmg_memcpy_h2d(h, ctypes.c_void_p(dV.ptr.value + 8 * j * N), col.ctypes.data, 8 * N))
        dw, dz, db, dx = ctx.to_device(rng.standard_normal(N)), ctx.alloc(N), ctx.to_device(b), ctx.alloc(N)
        out = ctypes.c_double(0.0)

        def dots_fused(k):
            return lambda: ctx.multi_dot(dV, dw, n=N, nvec=k, ld=N)

        def dots_single(k):
            def run():
                for j in range(k):
                    ctx.check(lib.aggmg_dot_dev(h, ctypes.c_void_p(dV.ptr.value + 8 * j * N), dw.ptr, N, ctypes.byref(out)))
            return run

        def update(k):
            c = np.full(k, 1e-9)       # (w stays finite over the repetitions)
            return lambda: ctx.multi_axpy_norm(dV, c, dw, n=N, nvec=k, ld=N)

        def frac(nbytes, ms):
            return {"TB_s": round(nbytes / (ms * 1e-3) / 1e12, 3), "of_8TBs": round(nbytes / (ms * 1e-3) / PEAK, 3),
                    "of_copy_ceiling": round(nbytes / (ms * 1e-3) / COPY, 3)}

        ortho = {}
        for k in sorted(set(args.nvec) | {1, 11, 30}):
            groups = [min(8, k - i) for i in range(0, k, 8)]
            bd = sum((g + 1) * 8 * N for g in groups)
            bu = sum((g + 2) * 8 * N for g in groups)
            td, tu, ts = timed(dots_fused(k)), timed(update(k)), timed(dots_single(k))
            ortho[k] = td + tu
            if k in args.nvec:
                print(json.dumps({"what": "passes", "log2_elems": E, "N": N, "nvec": k, "dots_ms": round(td, 4),
                                  "dots": frac(bd, td), "update_ms": round(tu, 4), "update": frac(bu, tu),
                                  "single_dots_ms": round(ts, 4), "fused_over_single": round(td / ts, 4)}), flush=True)
        for nPre, nPost in ((3, 3), (2, 1), (1, 1)):
            tc = timed(lambda: H.vcycle_dev(None, dw, dz, nPre, nPost))
            tr = timed(lambda: ctx.check(lib.aggmg_residual_dev(h, op.handle, dz.ptr, db.ptr, dx.ptr)))
            print(json.dumps({"what": "iteration", "log2_elems": E, "cycle": f"V({nPre},{nPost})", "cycle_ms": round(tc, 4),
                              "operator_ms": round(tr, 4),
                              "orthogonalisation_ms": {f"j={j}": round(ortho[j + 1], 4) for j in (0, 10, 29)},
                              "iteration_ms": {f"j={j}": round(tc + tr + ortho[j + 1], 4) for j in (0, 10, 29)}}), flush=True)
        for v in (dV, dw, dz):
            v.free()
        if not args.no_solve:
            hist = np.zeros(400)
            pd = ctypes.POINTER(ctypes.c_double)
            it, nchk = ctypes.c_int(0), ctypes.c_int(0)
            zero = ctx.alloc(N)

            def reset():
                ctx.check(lib.aggmg_copy_segments_dev(h, 1, (ctypes.c_void_p * 1)(zero.ptr.value),
                                                      (ctypes.c_void_p * 1)(dx.ptr.value), (ctypes.c_int64 * 1)(1),
                                                      (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N)))

            def solve(kind, nPre, nPost):
                def run():
                    reset()
                    if kind == "multigrid":
                        ctx.check(lib.aggmg_multigrid_dev(h, H.handle, zero.ptr, db.ptr, 400, 1e-8, 1, nPre, nPost, 2.0 / 3.0,
                                                          dx.ptr, hist.ctypes.data_as(pd), ctypes.byref(it), ctypes.byref(nchk),
                                                          None, None))
                    elif kind == "pcg":
                        ctx.check(lib.aggmg_pcg_dev(h, H.handle, db.ptr, dx.ptr, 400, 1e-8, nPre, nPost, 2.0 / 3.0,
                                                    hist.ctypes.data_as(pd), ctypes.byref(it)))
                    else:
                        ctx.check(lib.aggmg_fgmres_dev(h, H.handle, db.ptr, dx.ptr, args.restart, 400, 1e-8, nPre, nPost,
                                                       2.0 / 3.0, hist.ctypes.data_as(pd), ctypes.byref(it)))
                return run

            for cheb in (False, True):
                for kind, nPre, nPost in (("multigrid", 3, 3), ("pcg", 3, 3), ("fgmres", 3, 3), ("fgmres", 2, 1),
                                          ("fgmres", 1, 1)):
                    if cheb:
                        lam = H.estimate_lambda_max(0)
                        H.set_sweep_weights(0, mg.chebyshev_weights(lam, degree=nPre),
                                            mg.chebyshev_weights(lam, degree=nPost)[::-1])
                    ms = timed(solve(kind, nPre, nPost), reps=max(3, args.reps // 4), warm=1)
                    true = float(np.linalg.norm(mg.residual(op, dx.download(), b))) if E <= 22 else None
                    H.clear_sweep_weights()
                    print(json.dumps({"what": "solve", "log2_elems": E, "solver": kind, "cycle": f"V({nPre},{nPost})",
                                      "chebyshev_level0": cheb, "restart": args.restart if kind == "fgmres" else None,
                                      "iterations": it.value, "ms": round(ms, 3),
                                      "last_entry_over_b": float(hist[(nchk.value if kind == "multigrid" else it.value) - 1] / nb),
                                      "true_residual_over_b": None if true is None else true / nb}), flush=True)
            zero.free()
        for v in (db, dx):
            v.free()
        H.free()
    ctx.close()


if __name__ == "__main__":
    main()
