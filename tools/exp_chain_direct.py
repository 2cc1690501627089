#!/usr/bin/env python3
"""The direct solve of config 5's fine operator (CG p = 4 in the reference's vertices-first numbering) in element-chain
order on the device (AGGMG_COARSE_DEVICE_CHAIN), against the route it replaces: operator download, SciPy's SuperLU,
solve, upload.

    python tools/exp_chain_direct.py --log2-elems 20 --host-lu --out r.jsonl
    python tools/exp_chain_direct.py --log2-elems 22 24 --out r.jsonl

Per size, one JSON line: set-up time of the chain form (point-Jacobi smoother with the element lists) and of the
factorisation (aggmg_hier_create of the one-level hierarchy: pack, cyclic reduction, probe), device bytes the hierarchy
holds (device_memory() difference), the probe's backward error, ms per solve for one column and for a group of K columns
(wall clock around `reps` solves on rotating right-hand sides, synchronised at both ends), and the backward error
eta = ||b - A x|| / (||A||_inf ||x|| + ||b||) of the problem's own right-hand side.  --host-lu adds the parent's route,
timed in the same process.  A size whose factorisation is refused or does not fit is reported as such."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, nargs="+", default=[20])
    ap.add_argument("--p", type=int, default=4)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-lu", action="store_true", help="also time download + SuperLU + solve + upload")
    ap.add_argument("--out", help="append the JSON lines here")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.api import device_memory
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    ctx = mg.Context(0)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        r = fn()
        ctx.synchronize()
        return r, time.perf_counter() - t0

    for E in args.log2_elems:
        n = 2 ** E
        t0 = time.perf_counter()
        U = UniformCgDgHierarchy(n, ps=(args.p,))
        A = U.A[0]
        b = np.asarray(U.b, dtype=np.float64)
        N = A.shape[0]
        rec = {"log2_elems": E, "p": args.p, "N": int(N), "nnz": int(A.nnz), "host_assembly_s": time.perf_counter() - t0}
        print(f"# 2^{E}: operator assembled, N = {N}", flush=True)
        op, t = timed(lambda: mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx))
        rec["upload_s"] = t
        S, t = timed(lambda: mg.JacobiSmoother(op, ctx, U.element_nodes(0)))
        rec["chain_form_s"] = t
        m0 = device_memory()
        try:
            H, t = timed(lambda: mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=True, coarse_mode=_lib.COARSE_DEVICE_CHAIN))
        except _lib.AggmgError as e:
            rec["refused"] = str(e)
            emit(rec)
            continue
        rec["factor_s"] = t
        rec["device_bytes"] = device_memory()[1] - m0[1]
        rec["coarse_info"] = H.coarse_info()
        z = ctx.alloc(N)
        bd = [ctx.to_device(b), ctx.to_device(np.random.default_rng(E).standard_normal(N))]
        xd = ctx.alloc(N)

        def solves():
            for i in range(args.reps):
                H.vcycle_dev(z, bd[i % 2], xd, 0, 0, 1.0)
        solves()
        _, t = timed(solves)
        rec["solve_ms_K1"] = t * 1e3 / args.reps
        H.vcycle_dev(z, bd[0], xd, 0, 0, 1.0)
        x = xd.download()
        An = abs(A).sum(axis=1).max()
        rec["eta_own_rhs"] = float(np.linalg.norm(b - A @ x) / (An * np.linalg.norm(x) + np.linalg.norm(b)))
        rec["rel_residual_own_rhs"] = float(np.linalg.norm(b - A @ x) / np.linalg.norm(b))
        K = args.K
        try:
            dB = [mg.DeviceMatrix(ctx, N, K) for _ in range(2)]
            dX = mg.DeviceMatrix(ctx, N, K)

            def solves_k():
                for i in range(args.reps):
                    H.coarse_solve_multi_dev(dB[i % 2], dX)
            solves_k()
            _, t = timed(solves_k)
            rec[f"solve_ms_K{K}"] = t * 1e3 / args.reps
            rec["device_bytes_with_columns"] = device_memory()[1] - m0[1]
            for v in dB + [dX]:
                v.free()
        except _lib.AggmgError as e:
            rec[f"solve_ms_K{K}"] = None
            rec["columns_refused"] = str(e)
        if args.host_lu:
            t0 = time.perf_counter()
            Ah = op.to_scipy()
            rec["host_download_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            lu = spla.splu(Ah)
            rec["host_splu_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            bh = bd[0].download()
            xh = lu.solve(bh)
            u = ctx.to_device(xh)
            ctx.synchronize()
            rec["host_solve_roundtrip_ms"] = (time.perf_counter() - t0) * 1e3
            rec["eta_host_lu"] = float(np.linalg.norm(b - A @ xh) / (An * np.linalg.norm(xh) + np.linalg.norm(b)))
            rec["rel_diff_device_host"] = float(np.linalg.norm(x - xh) / np.linalg.norm(xh))
            del lu, Ah, u
        emit(rec)
        H.free(), S.free(), op.free()
        del U, A


if __name__ == "__main__":
    main()
