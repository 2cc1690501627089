#!/usr/bin/env python3
"""The coarsest direct solve of a column group: one launch sequence per group (cr_solve with kc columns) against the column loop.

    python tools/exp_multi_coarse.py --out new.jsonl                       # this checkout
    python tools/exp_multi_coarse.py --tree ../parent --out old.jsonl      # a checkout of the parent commit, same box
    python tools/exp_multi_coarse.py --table new.jsonl old.jsonl           # the markdown table of profiles/r11_multi_coarse.md

Systems: the config 3/4 hierarchy (DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1) at 2^20 and 2^24 fine elements, whose coarsest
level has 2^16 / 2^20 blocks of 2, and a one-level scalar system of 2^22 rows (config 5's coarsest shape, at a size that
fits with K = 8).  Per system and K in {1, 2, 4, 8}: ms of the coarsest solve of one group of K columns -- HIP events
(the library's profiler scopes, kind `coarse`) around the solves of a loop of K-column cycles on rotating right-hand
sides; a checkout that solves column by column opens one scope per column, and the K scopes of a cycle are summed -- and
the wall time of one whole K-column cycle.  The same script runs on both checkouts: it only uses entry points both have
(aggmg_vcycle_multi_dev; on a one-level hierarchy the cycle IS the coarsest solve).  One JSON line per (system, K)."""
import argparse
import json
import os
import sys
import time

import numpy as np


def measure(args):
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import scipy.sparse as sp
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib, uniform
    ctx = mg.Context(0)
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def run(name, H, sweeps):
        N = H._ops[0].shape[0]
        level = H.nlevels - 1
        Kmax = max(args.K)
        rng = np.random.default_rng(len(name))
        Bs = []
        B = rng.standard_normal((N, Kmax))      # (the same values in every buffer: the rotation is about what the caches hold)
        for _ in range(args.rotate):
            dB = mg.DeviceMatrix(ctx, N, Kmax)
            dB.upload(B)
            Bs.append(dB)
        del B
        dX = mg.DeviceMatrix(ctx, N, Kmax)
        for K in args.K:
            def cycle(i):
                H.vcycle_multi_dev(None, Bs[i % len(Bs)], dX, K, N, *sweeps)
            for i in range(3):
                cycle(i)
            ctx.synchronize()
            t0 = time.perf_counter()
            for i in range(args.reps):
                cycle(i)
            ctx.synchronize()
            ms_cycle = (time.perf_counter() - t0) * 1e3 / args.reps
            ctx.profile_enable(True)
            ctx.profile_collect()
            for i in range(args.reps):
                cycle(i)
            prof = ctx.profile_collect()
            ctx.profile_enable(False)
            c_ms, c_n = prof.get(("coarse", level), (0.0, 0))
            emit({"system": name, "rows_coarsest": int(H._ops[-1].shape[0]), "K": K, "reps": args.reps,
                  "coarse_ms_per_group": c_ms / args.reps, "coarse_scopes_per_cycle": c_n / args.reps,
                  "cycle_ms": ms_cycle, "coarse_info": H.coarse_info()})
        for v in Bs + [dX]:
            v.free()

    for E in args.log2_elems:
        U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
        H = uniform.build_device_hierarchy(U, ctx)
        run(f"dg_agg_2p{E}", H, (3, 3, 2.0 / 3.0))
        H.free()
    if args.scalar_log2:
        n = 2 ** args.scalar_log2
        # the DG p = 0 coarsest level's shape: a scaled 1-D Laplacian, Neumann end, Dirichlet penalty at the other
        d = np.full(n, 2.0 * n)
        d[0] = 1000.0 * n
        d[-1] = 1.0 * n
        A = sp.diags([np.full(n - 1, -1.0 * n), d, np.full(n - 1, -1.0 * n)], [-1, 0, 1], format="csc")
        op = mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx)
        try:
            H = mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_DEVICE_CR)
        except _lib.UnsupportedError as e:      # (the probe solve rejected the device factorisation)
            emit({"system": f"scalar_2p{args.scalar_log2}", "skipped": str(e)})
            return
        run(f"scalar_2p{args.scalar_log2}", H, (0, 0, 1.0))
        H.free()


def table(new_path, old_path):
    def load(p):
        return {(r["system"], r["K"]): r for r in map(json.loads, open(p)) if "K" in r}
    new, old = load(new_path), load(old_path)
    print("| system | K | column loop ms / group | batched ms / group | batched ms / column | ratio | coarsest share of the "
          "cycle, column loop | batched | cycle ms, column loop | batched |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for key in sorted(new):
        n, o = new[key], old[key]
        print(f"| {key[0]} | {key[1]} | {o['coarse_ms_per_group']:.4f} | {n['coarse_ms_per_group']:.4f} | "
              f"{n['coarse_ms_per_group'] / key[1]:.4f} | {n['coarse_ms_per_group'] / o['coarse_ms_per_group']:.3f} | "
              f"{o['coarse_ms_per_group'] / o['cycle_ms']:.3f} | {n['coarse_ms_per_group'] / n['cycle_ms']:.3f} | "
              f"{o['cycle_ms']:.4f} | {n['cycle_ms']:.4f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", help="the checkout whose package is measured (default: this file's)")
    ap.add_argument("--out", help="also write the JSON lines here")
    ap.add_argument("--log2-elems", type=int, nargs="*", default=[20, 24])
    ap.add_argument("--scalar-log2", type=int, default=22, help="rows of the one-level scalar system (0: skip)")
    ap.add_argument("--K", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rotate", type=int, default=3, help="right-hand-side matrices the loop rotates through")
    ap.add_argument("--table", nargs=2, metavar=("NEW", "OLD"), help="print the A/B table of two result files")
    args = ap.parse_args()
    if args.table:
        table(*args.table)
    else:
        measure(args)


if __name__ == "__main__":
    main()
