"""Launches per kind and level (the library's HIP-event profiler, aggmg_profile_collect) of the entry points that drive
cycles, on the benchmark's DG hierarchy and on a CG-chain hierarchy.  Two builds of the library that print the same
table launch the same sequence -- what a host-side refactor has to show (AGGMG_HIP_LIB picks the build).

    python tools/launch_counts.py [--log2-elems E] [--cg-elems N]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import agglomerationmultigrid1d_amd as mg  # noqa: E402
from agglomerationmultigrid1d_amd.api import multigrid_dev, smoother_solve_dev  # noqa: E402
from agglomerationmultigrid1d_amd.uniform import (UniformCgDgHierarchy, UniformDgAggHierarchy,  # noqa: E402
                                                  build_device_cg_hierarchy, build_device_hierarchy)


def void(_):
    return None


def table(name, ctx, fn):
    ctx.synchronize()
    ctx.profile_enable(True)
    note = fn()
    ctx.profile_enable(False)
    prof = ctx.profile_collect()
    cells = " ".join(f"{kind}@{lvl}={cnt}" for (kind, lvl), (_, cnt) in sorted(prof.items()))
    print(f"{name:34s} {note or '':22s} {cells}", flush=True)


def cases(tag, H, b_host, multi):
    ctx = H.ctx
    N = len(b_host)
    b = ctx.to_device(b_host)
    x0 = ctx.to_device(np.zeros(N))
    out = ctx.alloc(N)
    table(f"{tag} multigrid_v_cycle", ctx, lambda: void(mg.multigrid_v_cycle(H, x0, b)))
    table(f"{tag} vcycles_dev ncycles=5", ctx, lambda: void(H.vcycles_dev(x0, b, out, 5)))
    for ce in (1, 3):
        for tol in (1e-30, 1e-4):   # to maxiter, and stopped by the tolerance between two cycles
            def run(ce=ce, tol=tol):
                r = multigrid_dev(H, x0, b, 7, tol, ce)
                return f"cycles={r[1]} checks={len(r[2])}"
            table(f"{tag} multigrid ce={ce} tol={tol:g}", ctx, run)
    for ce in (1, 3):
        def run(ce=ce):
            r = smoother_solve_dev(H._ops[0], H.mSmoothers[0], x0, b, 20, 1e-30, 2.0 / 3.0, ce)
            return f"iters={r[1]} checks={len(r[2])}"
        table(f"{tag} smoother_solve ce={ce}", ctx, run)
    if multi:
        B = np.stack([b_host * (j + 1) for j in range(4)], axis=1)
        table(f"{tag} multigrid_v_cycle K=4", ctx, lambda: void(mg.multigrid_v_cycle(H, np.zeros_like(B), B)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=16, help="fine DG elements of the benchmark's hierarchy (counts do not depend on it)")
    ap.add_argument("--cg-elems", type=int, default=1000)
    args = ap.parse_args()
    ctx = mg.Context()
    U = UniformDgAggHierarchy(2 ** args.log2_elems, p=3, pAgg=1, ratios=(4, 2, 2))
    H = build_device_hierarchy(U, ctx)
    print("dg levels:", H.level_kinds())
    cases("dg", H, U.rhs(), True)
    H.free()
    U = UniformCgDgHierarchy(args.cg_elems, ps=(4, 2, 1))
    H = build_device_cg_hierarchy(U, ctx)
    print("cg levels:", H.level_kinds())
    cases("cg", H, U.rhs(), False)
    H.free()


if __name__ == "__main__":
    main()
