#!/usr/bin/env python3
"""K right-hand sides per V-cycle (aggmg_vcycle_multi_dev) against K single-vector cycles, on the config 3/4 hierarchy
(DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1), zero initial guesses (ldiv!):

    python tools/exp_multi_rhs.py [--log2-elems 22 24] [--K 1 2 4 8] [--reps 7]
    python tools/exp_multi_rhs.py --profile-only K --log2-elems 24      # the command rocprofv3 runs (one K, no timing)
    python tools/exp_multi_rhs.py --multi-elem 0                        # AGGMG_OPT_MULTI_ELEMENT_THREADS off (default: as built)
    AGGMG_HIP_LIB=old/libaggmg_hip.so python tools/exp_multi_rhs.py     # a build from before that option: its symbols dropped

Per size and K: ms of one K-column cycle and of K single cycles (timed alternately in one process, medians), ms per
column and the ratio, fine-level DoF-updates/s, and the fine K-column descent's compulsory-bytes fraction of 8 TB/s
(aggmg_hier_multi_launch_bytes over the launch's HIP-event time, profiling mode 2), the fine K-column ascent's time
(profiling mode 1) and the launches of the K-column element-thread kernel.  One JSON line per (size, K)."""
import argparse
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
    ap.add_argument("--profile-only", type=int, default=0, metavar="K",
                    help="run 1 warm-up + 3 K-column cycles and nothing else (for rocprofv3)")
    ap.add_argument("--multi-elem", type=int, choices=(0, 1), default=None,
                    help="set AGGMG_OPT_MULTI_ELEMENT_THREADS (default: the library's)")
    args = ap.parse_args()
    import ctypes
    from agglomerationmultigrid1d_amd import _lib
    # a library from before AGGMG_OPT_MULTI_ELEMENT_THREADS (AGGMG_HIP_LIB, the other arm of a comparison) lacks its symbols
    probe = ctypes.CDLL(_lib.LIB_PATH)
    has_multi_elem = hasattr(probe, "aggmg_multi_element_thread_launches")
    if not has_multi_elem:
        for name in [n for n in _lib.SYMBOLS if "multi_element" in n]:
            del _lib.SYMBOLS[name]
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import uniform
    ctx = mg.Context(0)
    if args.multi_elem is not None and has_multi_elem:
        ctx.set_option(_lib.OPT_MULTI_ELEMENT_THREADS, args.multi_elem)
    for E in args.log2_elems:
        U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
        H = uniform.build_device_hierarchy(U, ctx)
        N = H._ops[0].shape[0]
        Kmax = args.profile_only or max(args.K)
        rng = np.random.default_rng(E)
        dB = mg.DeviceMatrix(ctx, N, Kmax)
        dB.upload(rng.standard_normal((N, Kmax)))
        dX = mg.DeviceMatrix(ctx, N, Kmax)
        xo = ctx.alloc(N)
        base = dB.ptr.value

        if args.profile_only:
            for _ in range(4):
                H.vcycle_multi_dev(None, dB, dX, Kmax, N)
            ctx.synchronize()
            print(json.dumps({"log2_elems": E, "K": Kmax, "multi_info": H.multi_info(Kmax)}))
            H.free()
            continue

        def multi(K):
            H.vcycle_multi_dev(None, dB, dX, K, N)

        def single(K):
            for j in range(K):
                H.vcycle_dev(None, base + 8 * j * N, xo)

        def timed(fn, K):
            ctx.synchronize()
            t0 = time.perf_counter()
            fn(K)
            ctx.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for K in args.K:
            fused, group = H.multi_info(K)
            multi(K)
            single(K)
            tm, ts = [], []
            for _ in range(args.reps):   # alternating
                tm.append(timed(multi, K))
                ts.append(timed(single, K))
            ms_m, ms_s = float(np.median(tm)), float(np.median(ts))
            # the fine K-column descent alone: one event pair per cycle (profiling mode 2)
            ctx.synchronize()
            ctx.profile_enable(2)
            for _ in range(args.reps):
                multi(K)
            st = ctx.profile_collect()
            ctx.profile_enable(False)
            d_ms, d_n = st.get(("fused_down", 0), (0.0, 0))
            ctx.profile_enable(1)   # every launch: the fine ascent
            for _ in range(args.reps):
                multi(K)
            st = ctx.profile_collect()
            ctx.profile_enable(False)
            u_ms, u_n = st.get(("fused_up", 0), (0.0, 0))
            k0 = ctx.multi_element_thread_launches() if has_multi_elem else 0
            multi(K)
            ctx.synchronize()
            elem = (ctx.multi_element_thread_launches() - k0) if has_multi_elem else 0
            ngroups = -(-K // group)
            rd, wr = 0, 0
            for c0 in range(0, K, group):
                r_, w_ = H.multi_launch_bytes(0, "down", min(group, K - c0), has_x0=False)
                rd, wr = rd + r_, wr + w_
            d_one = d_ms / max(d_n, 1) * ngroups   # ms of the fine descent launches of one cycle
            frac = (rd + wr) / (d_one * 1e-3) / PEAK if d_one > 0 else 0.0
            print(json.dumps({
                "log2_elems": E, "K": K, "fused": fused, "group": group,
                "ms_multi": round(ms_m, 4), "ms_single_xK": round(ms_s, 4),
                "ms_per_col_multi": round(ms_m / K, 4), "ms_per_col_single": round(ms_s / K, 4),
                "per_col_ratio": round(ms_m / ms_s, 4),
                "fine_dof_updates_per_s_multi": N * K / (ms_m * 1e-3), "fine_dof_updates_per_s_single": N * K / (ms_s * 1e-3),
                "multi_elem_launches_per_cycle": elem,
                "fine_descent_ms": round(d_one, 4), "fine_ascent_ms": round(u_ms / max(u_n, 1) * ngroups, 4), "fine_descent_bytes": rd + wr,
                "fine_descent_frac_8TBs": round(frac, 4),
                "coarse_ms_per_col": round(H.last_coarse_ms(), 4)}), flush=True)
        for v in (dB, dX, xo):
            v.free()
        H.free()


if __name__ == "__main__":
    main()
