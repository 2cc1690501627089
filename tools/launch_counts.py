"""Launches per kind and level (the library's HIP-event profiler, aggmg_profile_collect) of the entry points that drive
cycles: on the benchmark's DG hierarchy and a CG-chain hierarchy (every level fused), and on small hierarchies that reach
the rest of the cycle driver -- generic CSR sweeps, block sweeps on overlapping and on scrambled lists, the band kernel,
block Gauss-Seidel, chunked block-tridiagonal sweeps between generic transfers, agglomerates of different sizes,
element-patch levels (hybrid, additive and multiplicative).  Every hierarchy also runs a cycle on K = 11 columns with the
opt-in column-group paths on (AGGMG_OPT_PATCH_MULTI, AGGMG_OPT_CHAIN_MULTI: groups of 8 and 3 columns where the levels
qualify, column by column elsewhere) and the K-column residual of its fine operator.  Two
builds of the library that print the same table launch the same sequence, and with --dump the vectors they computed can
be compared byte for byte -- what a host-side refactor has to show (AGGMG_HIP_LIB picks the build).

    python tools/launch_counts.py [--log2-elems E] [--cg-elems N] [--small-elems N] [--dump DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import agglomerationmultigrid1d_amd as mg  # noqa: E402
from agglomerationmultigrid1d_amd import _lib  # noqa: E402
from agglomerationmultigrid1d_amd.api import multigrid_dev, smoother_solve_dev  # noqa: E402
from agglomerationmultigrid1d_amd.uniform import (UniformCgDgHierarchy, UniformDgAggHierarchy,  # noqa: E402
                                                  build_device_cg_hierarchy, build_device_hierarchy,
                                                  build_device_ragged_hierarchy)

DUMP = None


def table(name, ctx, fn):
    """fn() -> (note, result: DeviceVector / array / None)"""
    ctx.synchronize()
    ctx.profile_enable(True)
    note, x = fn()
    ctx.profile_enable(False)
    prof = ctx.profile_collect()
    cells = " ".join(f"{kind}@{lvl}={cnt}" for (kind, lvl), (_, cnt) in sorted(prof.items()))
    print(f"{name:34s} {note or '':22s} {cells}", flush=True)
    if DUMP and x is not None:
        x = x if isinstance(x, np.ndarray) else x.download()
        np.save(os.path.join(DUMP, name.replace(" ", "_").replace("=", "") + ".npy"), x)


def cases(tag, H, b_host, multi):
    ctx = H.ctx
    N = len(b_host)
    b = ctx.to_device(b_host)
    x0 = ctx.to_device(np.zeros(N))
    out = ctx.alloc(N)
    table(f"{tag} multigrid_v_cycle", ctx, lambda: (None, mg.multigrid_v_cycle(H, x0, b)))

    def vcycles():
        H.vcycles_dev(x0, b, out, 5)
        return None, out
    table(f"{tag} vcycles_dev ncycles=5", ctx, vcycles)
    for ce in (1, 3):
        for tol in (1e-30, 1e-4):   # to maxiter, and stopped by the tolerance between two cycles
            def run(ce=ce, tol=tol):
                r = multigrid_dev(H, x0, b, 7, tol, ce)
                return f"cycles={r[1]} checks={len(r[2])}", r[0]
            table(f"{tag} multigrid ce={ce} tol={tol:g}", ctx, run)
    for ce in (1, 3):
        def run(ce=ce):
            r = smoother_solve_dev(H._ops[0], H.mSmoothers[0], x0, b, 20, 1e-30, 2.0 / 3.0, ce)
            return f"iters={r[1]} checks={len(r[2])}", r[0]
        table(f"{tag} smoother_solve ce={ce}", ctx, run)
    if multi:
        B = np.stack([b_host * (j + 1) for j in range(4)], axis=1)
        table(f"{tag} multigrid_v_cycle K=4", ctx, lambda: (None, mg.multigrid_v_cycle(H, np.zeros_like(B), B)))


def multi_cases(tag, H, b_host, K=11):
    """the K-column entry points with the opt-in column-group paths on"""
    ctx = H.ctx
    N = len(b_host)
    B = np.stack([b_host * (j + 1) for j in range(K)], axis=1)
    X0 = np.stack([np.cos(np.arange(N) * (0.37 + 0.05 * j)) for j in range(K)], axis=1)
    for opt in (_lib.OPT_PATCH_MULTI, _lib.OPT_CHAIN_MULTI):
        ctx.set_option(opt, 1)
    try:
        fused, group = H.multi_info(K)
        table(f"{tag} vcycle K={K}", ctx, lambda: (f"fused={int(fused)} group={group}", mg.multigrid_v_cycle(H, X0, B)))

        def residual():
            dX, dB, dR = (mg.DeviceMatrix(ctx, N, K) for _ in range(3))
            dX.upload(np.asfortranarray(X0))
            dB.upload(np.asfortranarray(B))
            H._ops[0].residual_multi_dev(dX, dB, dR)
            R = dR.download()
            for v in (dX, dB, dR):
                v.free()
            return None, R
        table(f"{tag} residual_multi K={K}", ctx, residual)
    finally:
        for opt in (_lib.OPT_PATCH_MULTI, _lib.OPT_CHAIN_MULTI):
            ctx.set_option(opt, 0)


# ---- small hierarchies off the all-fused path: name -> (build(ctx, n) -> (H, b), level kinds, main sweep counts) ----
def _cg(smoother):
    def build(ctx, n):
        U = UniformCgDgHierarchy(n, ps=(4, 2, 1))
        if smoother == "jac":   # chain detection off: generic CSR sweeps, one per launch
            return build_device_cg_hierarchy(U, ctx, chain=False), U.rhs()
        # element Schwarz on lists in a scrambled order (not the chain): block sweep + combine
        cls = {"addSchwarz": mg.AdditiveSchwarzSmoother, "hybridSchwarz": mg.HybridSchwarzSmoother}[smoother]
        ops = [mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx) for A in U.A]
        sms = []
        for k in range(U.nlevels - 1):
            el = U.element_nodes(k)
            sms.append(cls(ops[k], np.ascontiguousarray(el[:, np.random.default_rng(k).permutation(el.shape[1])]), ctx))
        Ls = [mg.DeviceOperator(L, _lib.OP_TRANSFER, ctx) for L in U.L]
        return mg.MeshHierarchy(None, ops, sms, Ls, ctx=ctx), U.rhs()
    return build


def _dg(smoother):
    def build(ctx, n):
        U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=(4, 2, 2))
        if smoother in ("blockJac", "blockGS", "patchSchwarz0", "patchGS0"):
            return build_device_hierarchy(U, ctx, smoother=smoother), U.rhs()
        ops = [mg.DeviceOperator(U.stiffness_csc(k), _lib.OP_STIFFNESS, ctx) for k in range(U.nlevels)]
        if smoother == "jac":   # banded operators under point Jacobi: the band kernel, residual out of the sweeps' launch
            sms = [mg.JacobiSmoother(op, ctx, detect=False) for op in ops[:-1]]
        elif smoother == "patchAdd0":   # additive element patches on the fine level, block Jacobi below
            inds = [U.descriptor(k).mBlockInds for k in range(U.nlevels - 1)]
            sms = [mg.ElementPatchSchwarz(ops[0], inds[0].shape[0], inds[0].shape[1], hybrid=False, ctx=ctx)]
            sms += [mg.BlockJacobi(ops[k], inds[k], ctx) for k in range(1, U.nlevels - 1)]
        else:                   # the elements' blocks in a scrambled order: a partition of the rows, the one-pass block sweep
            sms = []
            for k in range(U.nlevels - 1):
                inds = U.descriptor(k).mBlockInds
                sms.append(mg.BlockJacobi(ops[k], np.ascontiguousarray(inds[:, np.random.default_rng(k).permutation(inds.shape[1])]), ctx))
        Ls = [mg.DeviceOperator(U.interpolation_csc(k), _lib.OP_TRANSFER, ctx) for k in range(U.nlevels - 1)]
        meshes = [U.descriptor(k) for k in range(U.nlevels)] if smoother == "patchAdd0" else None   # (as build_device_hierarchy)
        return mg.MeshHierarchy(meshes, ops, sms, Ls, ctx=ctx), U.rhs()
    return build


def _ragged(ctx, n):
    H, b, _ = build_device_ragged_hierarchy(n, ctx, p=3, seed=3)
    return H, b


GENERIC, BTD = ["generic"] * 3 + ["coarsest"], ["fused_btd"] * 3 + ["coarsest"]
SMALL = {
    "cg_jac": (_cg("jac"), GENERIC, (3, 3)),
    "cg_add": (_cg("addSchwarz"), GENERIC, (3, 3)),
    "cg_hyb": (_cg("hybridSchwarz"), GENERIC, (3, 3)),
    "dg_band": (_dg("jac"), GENERIC, (3, 3)),
    "dg_scr": (_dg("scrambled"), GENERIC, (3, 3)),
    "dg_gs": (_dg("blockGS"), BTD, (3, 3)),
    "dg_s12": (_dg("blockJac"), BTD, (12, 12)),   # more sweeps than a fused launch takes: chunks + generic transfers
    "ragged": (_ragged, BTD, (3, 3)),
    "patch_hyb": (_dg("patchSchwarz0"), BTD, (3, 3)),
    "patch_add": (_dg("patchAdd0"), BTD, (3, 3)),
    "patch_gs": (_dg("patchGS0"), BTD, (3, 3)),
    "patch_gs12": (_dg("patchGS0"), BTD, (12, 12)),   # more sweeps than a patch launch takes: chunks
}


def small_cases(tag, H, b_host, sweeps):
    ctx = H.ctx
    N = len(b_host)
    b = ctx.to_device(b_host)
    x0 = ctx.to_device(np.cos(np.arange(N) * 0.37))

    def cycle(nPre, nPost):
        out = ctx.alloc(N)
        H.vcycle_dev(x0, b, out, nPre, nPost, 0.5)
        return None, out
    for nPre, nPost in (sweeps, (0, 2), (2, 0)):
        table(f"{tag} vcycle ({nPre},{nPost})", ctx, lambda: cycle(nPre, nPost))

    def vcycles():
        out = ctx.alloc(N)
        H.vcycles_dev(x0, b, out, 3, sweeps[0], sweeps[1], 0.5)
        return None, out
    table(f"{tag} vcycles_dev ncycles=3", ctx, vcycles)

    def multigrid():
        r = multigrid_dev(H, x0, b, 5, 1e-30, 2, sweeps[0], sweeps[1], 0.5)
        return f"cycles={r[1]} checks={len(r[2])}", r[0]
    table(f"{tag} multigrid ce=2", ctx, multigrid)

    def smoother_solve():
        r = smoother_solve_dev(H._ops[0], H.mSmoothers[0], x0, b, 7, 1e-30, 0.5, 3)
        return f"iters={r[1]} checks={len(r[2])}", r[0]
    table(f"{tag} smoother_solve ce=3", ctx, smoother_solve)
    # a sweep-weight schedule on the two finest levels (the schedules hold at most 8 weights per half)
    H.set_sweep_weights(0, [0.3, 0.5, 0.7], [0.6, 0.4, 0.2])
    H.set_sweep_weights(1, [0.45, 0.55, 0.65])
    table(f"{tag} scheduled vcycle (3,3)", ctx, lambda: cycle(3, 3))

    def scheduled_vcycles():
        out = ctx.alloc(N)
        H.vcycles_dev(x0, b, out, 3, 3, 3, 0.5)
        return None, out
    table(f"{tag} scheduled vcycles_dev", ctx, scheduled_vcycles)
    H.clear_sweep_weights()


def main():
    global DUMP
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=16, help="fine DG elements of the benchmark's hierarchy (counts do not depend on it)")
    ap.add_argument("--cg-elems", type=int, default=1000)
    ap.add_argument("--small-elems", type=int, default=384, help="fine elements of the small hierarchies")
    ap.add_argument("--dump", metavar="DIR", help="write every case's result vector to DIR/<case>.npy")
    args = ap.parse_args()
    if args.dump:
        DUMP = args.dump
        os.makedirs(DUMP, exist_ok=True)
    ctx = mg.Context()
    U = UniformDgAggHierarchy(2 ** args.log2_elems, p=3, pAgg=1, ratios=(4, 2, 2))
    H = build_device_hierarchy(U, ctx)
    print("dg levels:", H.level_kinds())
    cases("dg", H, U.rhs(), True)
    multi_cases("dg", H, U.rhs())
    H.free()
    U = UniformCgDgHierarchy(args.cg_elems, ps=(4, 2, 1))
    H = build_device_cg_hierarchy(U, ctx)
    print("cg levels:", H.level_kinds())
    cases("cg", H, U.rhs(), False)
    multi_cases("cg", H, U.rhs())
    H.free()
    for tag, (build, kinds, sweeps) in SMALL.items():
        H, b = build(ctx, args.small_elems)
        print(f"{tag} levels:", H.level_kinds())
        assert H.level_kinds() == kinds, (tag, H.level_kinds(), kinds)
        small_cases(tag, H, b, sweeps)
        multi_cases(tag, H, b)
        H.free()
    # (the one line that differs between a build with AGGMG_OPT_COARSE_DICTIONARY and one without or before it)
    if hasattr(ctx, "coarse_dictionary_launches"):
        print("coarse dictionary launches:", ctx.coarse_dictionary_launches())


if __name__ == "__main__":
    main()
