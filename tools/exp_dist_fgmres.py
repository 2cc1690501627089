"""The fused owned-range passes of distributed.fgmres against the calls they replace, and the partitioned loop on ONE rank
against the single-GPU loop -- on one GPU, nothing through thread ranks.

  1. aggmg_owned_multi_dot_dev (one pass over w per group of 8 vectors, one read-back) against nvec calls of
     aggmg_owned_dot_dev; aggmg_owned_multi_axpy_norm_dev against nvec one-vector update passes and an owned dot for the
     norm.  Local lengths 2^22 and 2^24 doubles, nvec = 8, 16, 30, the owned range the vector without 1000 rows at either
     end.  The two forms ALTERNATE, `--reps` times; per form the median and the spread (max - min) of the repetitions.
     The fused form "wins" when its median is below the baseline's by more than three times the baseline's spread.
     Bandwidth: the bytes the pass must move (every basis vector once, w once per group -- read for the dots, read and
     written for the update) over the median, beside the 8 TB/s peak and a device-to-device copy of the same length
     measured here (read + write bytes over its median).
  2. distributed.fgmres on a world of one rank (the whole domain is owned: no ghosts, every exchange a no-op) against
     mg.fgmres on the patchSchwarz0 hierarchy at 2^20 and 2^22 elements, V(3,3), restart 30, tol 1e-8.  Reported only.

    python tools/exp_dist_fgmres.py [--lengths 22 24] [--nvecs 8 16 30] [--reps 15] [--solver-log2 20 22] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBS = 8000.0


def _arr(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*[int(v) for v in vals])


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def alternate(forms, reps, sync):
    """forms: {name: callable}; every repetition runs each once, in turn -> {name: (median s, spread s)}"""
    times = {k: [] for k in forms}
    for k, fn in forms.items():            # warm-up: code objects, buffers
        fn()
    sync()
    for _ in range(reps):
        for k, fn in forms.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            times[k].append(time.perf_counter() - t0)
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in times.items()}


def passes(ctx, torch, log2n, nvecs, reps):
    n = 2 ** log2n
    lo, hi = _arr([1000]), _arr([n - 1000])
    ld = n
    V = torch.randn((max(nvecs), ld), dtype=torch.float64, device="cuda") * 1e-3
    w = torch.randn(n, dtype=torch.float64, device="cuda")
    w2 = torch.empty_like(w)
    sync = torch.cuda.synchronize
    lib, h = ctx.lib, ctx.handle
    one = ctypes.c_double(0.0)
    pd = ctypes.POINTER(ctypes.c_double)
    copy = alternate({"copy": lambda: w2.copy_(w)}, reps, sync)["copy"]
    rows = {"log2_length": log2n, "copy_GBs": 2 * n * 8 / copy[0] / 1e9, "copy_ms": 1e3 * copy[0], "nvec": {}}
    for nvec in nvecs:
        out = np.zeros(nvec)
        coef = np.full(nvec, 1e-3)
        groups = (nvec + 7) // 8

        def fused_dot():
            ctx.check(lib.aggmg_owned_multi_dot_dev(h, _P(V), nvec, ld, _P(w), 1, lo, hi, out.ctypes.data_as(pd)))

        def single_dots():
            for i in range(nvec):
                ctx.check(lib.aggmg_owned_dot_dev(h, _P(w), _P(V[i]), 1, lo, hi, ctypes.byref(one)))

        def fused_axpy():
            ctx.check(lib.aggmg_owned_multi_axpy_norm_dev(h, n, _P(V), nvec, ld, coef.ctypes.data_as(pd), _P(w), 1, lo, hi,
                                                          ctypes.byref(one)))

        def single_axpys():
            for i in range(nvec):
                ctx.check(lib.aggmg_owned_multi_axpy_norm_dev(h, n, _P(V[i]), 1, ld, coef[i:].ctypes.data_as(pd), _P(w), 1, lo, hi,
                                                              None))
            ctx.check(lib.aggmg_owned_dot_dev(h, _P(w), _P(w), 1, lo, hi, ctypes.byref(one)))

        t = alternate({"fused_dot": fused_dot, "single_dots": single_dots}, reps, sync)
        t.update(alternate({"fused_axpy": fused_axpy, "single_axpys": single_axpys}, reps, sync))
        bytes_dot = (nvec + groups) * n * 8
        bytes_axpy = (nvec + 2 * groups) * n * 8
        row = {}
        for fused, base, nbytes in (("fused_dot", "single_dots", bytes_dot), ("fused_axpy", "single_axpys", bytes_axpy)):
            (mf, sf), (mb, sb) = t[fused], t[base]
            row[fused] = {"ms": 1e3 * mf, "spread_ms": 1e3 * sf, "baseline": base, "baseline_ms": 1e3 * mb,
                          "baseline_spread_ms": 1e3 * sb, "speedup": mb / mf, "wins_by_3_spreads": bool(mb - mf > 3 * sb),
                          "GBs": nbytes / mf / 1e9, "frac_of_peak": nbytes / mf / 1e9 / PEAK_GBS,
                          "frac_of_copy": nbytes / mf / 1e9 / rows["copy_GBs"]}
        rows["nvec"][str(nvec)] = row
    return rows


def solvers(mg, torch, log2n, tol):
    from agglomerationmultigrid1d_amd import distributed as D
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    n, p, ratios = 2 ** log2n, 3, (4, 2, 2)
    kw = dict(restart=30, maxiter=100, tol=tol, nPre=3, nPost=3)
    ctx = mg.Context(0)
    Ug = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios)
    Hg = build_device_hierarchy(Ug, ctx, smoother="patchSchwarz0")
    bg = ctx.to_device(np.array(Ug.rhs()))
    mg.fgmres(Hg, bg, **dict(kw, maxiter=2))                  # warm-up, work space
    ctx.synchronize()
    t0 = time.perf_counter()
    _, it_g, res_g = mg.fgmres(Hg, bg, **kw)
    ctx.synchronize()
    t_g = time.perf_counter() - t0
    Hg.free()
    del bg
    comm = D.ThreadComm(D.ThreadGroup(1), 0)                  # a world of one rank: no thread, no collective waits
    ctx1 = mg.Context(0)
    layout = D.RankLayout(n, ratios, [p + 1, 2, 2, 2], 1, 0, smoothers=D.smoother_kinds("patchSchwarz0", len(ratios)))
    engine, U = D.build_local_uniform(n, p, 1, ratios, layout, ctx1, comm, smoother="patchSchwarz0")
    dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
    b = torch.from_numpy(np.array(U.rhs())).to(engine.dev)
    D.fgmres(dv, b, **dict(kw, maxiter=2))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, it_d, res_d = D.fgmres(dv, b, **kw)
    torch.cuda.synchronize()
    t_d = time.perf_counter() - t0
    dv.free()
    return {"log2_elems": log2n, "tol": tol, "single_gpu": {"iterations": it_g, "ms": 1e3 * t_g, "final_res": res_g[-1]},
            "partitioned_world_1": {"iterations": it_d, "ms": 1e3 * t_d, "final_res": res_d[-1]},
            "ms_per_iteration": {"single_gpu": 1e3 * t_g / max(it_g, 1), "partitioned_world_1": 1e3 * t_d / max(it_d, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="*", default=[22, 24], help="log2 of the local vector lengths of part 1")
    ap.add_argument("--nvecs", type=int, nargs="*", default=[8, 16, 30])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--solver-log2", type=int, nargs="*", default=[20, 22], help="log2 of the element counts of part 2")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import agglomerationmultigrid1d_amd as mg
    if not torch.cuda.is_available():
        sys.exit("exp_dist_fgmres: no GPU (nothing here is measured without one)")
    ctx = mg.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    out = {"passes": [passes(ctx, torch, l2, args.nvecs, args.reps) for l2 in args.lengths],
           "solvers": [solvers(mg, torch, l2, args.tol) for l2 in args.solver_log2]}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
