#!/usr/bin/env python3
"""The K-column cycle on CG chain levels (AGGMG_OPT_CHAIN_MULTI) against the column-by-column cycle it replaces, on the
config-5 hierarchy CG p = 4 -> 2 -> 1 -> DG p = 0 (UniformCgDgHierarchy), zero initial guesses:

    python tools/exp_chain_multi.py --log2-elems 20 [--K 2 4 8] [--reps 9] [--dictionary 1]

One process per size and dictionary setting: run each under a time limit of its own.  Both sides are the SAME call,
vcycle_multi_dev V(3,3) on the same hierarchy and buffers, with the option on and off (it is read at every call); a
warm-up of both, then the two timed alternately, medians with the smallest and largest time.  pcg on N x 8 (10
iterations, tolerance 0) the same way.  Per K one JSON line: ms per cycle and per column on either side, the ratio
on / off, and the two launches of the p = 4 level of one cycle on either side (HIP-event time, profiling on, a run of its
own) with the compulsory bytes aggmg_hier_multi_launch_bytes / aggmg_hier_launch_bytes count for them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=20)
    ap.add_argument("--K", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dictionary", type=int, default=1)
    ap.add_argument("--pcg-iters", type=int, default=10)
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib, uniform
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, args.dictionary)
    E = args.log2_elems
    U = uniform.UniformCgDgHierarchy(2 ** E)
    H = uniform.build_device_cg_hierarchy(U, ctx)
    assert H.level_kinds() == ["fused_chain"] * 3 + ["coarsest"], H.level_kinds()
    N = H._ops[0].shape[0]
    Kmax = max(max(args.K), 8)
    rng = np.random.default_rng(E)
    dB = mg.DeviceMatrix(ctx, N, Kmax)
    dB.upload(np.asfortranarray(rng.standard_normal((N, Kmax))))
    dX = mg.DeviceMatrix(ctx, N, Kmax)
    zeros = np.zeros((N, Kmax), order="F")
    classes = H.dictionary_levels()

    def option(on):
        ctx.set_option(_lib.OPT_CHAIN_MULTI, 1 if on else 0)

    def timed(fn):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def ab(fn):
        """median ms of fn with the option on and off, timed alternately after a warm-up of both"""
        t = {True: [], False: []}
        for on in (True, False):
            option(on)
            fn()
        for _ in range(args.reps):
            for on in (True, False):
                option(on)
                t[on].append(timed(fn))
        return float(np.median(t[True])), float(np.median(t[False])), t

    for K in args.K:
        option(True)
        fused, group = H.multi_info(K)
        ms_on, ms_off, t = ab(lambda: H.vcycle_multi_dev(None, dB, dX, K, N))
        # the p = 4 level's two launches of one cycle on either side: event time, in a run of its own
        fine_ms, fine_n, launches = {}, {}, 0
        for on in (True, False):
            option(on)
            ctx.synchronize()
            before = ctx.chain_multi_launches()
            ctx.profile_enable(1)
            for _ in range(args.reps):
                H.vcycle_multi_dev(None, dB, dX, K, N)
            st = ctx.profile_collect()
            ctx.profile_enable(False)
            if on:
                launches = (ctx.chain_multi_launches() - before) // args.reps
            d_ms, d_n = st.get(("fused_down", 0), (0.0, 0))
            u_ms, u_n = st.get(("fused_up", 0), (0.0, 0))
            fine_ms[on], fine_n[on] = (d_ms + u_ms) / args.reps, (d_n + u_n) // args.reps
        bytes_on = 0
        for c0 in range(0, K, group):
            kc = min(group, K - c0)
            bytes_on += sum(sum(H.multi_launch_bytes(0, kind, kc, has_x0=False)) for kind in ("down", "up"))
        bytes_off = K * sum(sum(H.multi_launch_bytes(0, kind, 1, has_x0=False)) for kind in ("down", "up"))
        print(json.dumps({
            "log2_elems": E, "dictionary": args.dictionary, "dictionary_classes": classes, "K": K, "fused_on": fused, "group": group,
            "ms_on": round(ms_on, 4), "ms_off": round(ms_off, 4), "ms_per_col_on": round(ms_on / K, 4),
            "ms_per_col_off": round(ms_off / K, 4), "ratio_on_off": round(ms_on / ms_off, 4),
            "spread_on": [round(min(t[True]), 4), round(max(t[True]), 4)], "spread_off": [round(min(t[False]), 4), round(max(t[False]), 4)],
            "chain_multi_launches_per_cycle": int(launches), "fine_launches_on": int(fine_n[True]), "fine_launches_off": int(fine_n[False]),
            "fine_ms_on": round(fine_ms[True], 4), "fine_ms_off": round(fine_ms[False], 4), "fine_bytes_on": int(bytes_on),
            "fine_bytes_off": int(bytes_off),
            "fine_TBps_on": round(bytes_on / (fine_ms[True] * 1e-3) / 1e12, 4) if fine_ms[True] > 0 else None,
            "fine_TBps_off": round(bytes_off / (fine_ms[False] * 1e-3) / 1e12, 4) if fine_ms[False] > 0 else None}), flush=True)

    # pcg on N x 8, a fixed number of iterations from zero guesses
    K = 8

    def pcg():
        H.pcg_multi_dev(dB, dX, K, N, maxiter=args.pcg_iters, tol=0.0)

    t = {True: [], False: []}
    for rep in range(-1, max(3, args.reps // 2)):   # (rep -1: warm-up)
        for on in (True, False):
            option(on)
            dX.upload(zeros)
            ms = timed(pcg)
            if rep >= 0:
                t[on].append(ms)
    ms_on, ms_off = float(np.median(t[True])), float(np.median(t[False]))
    print(json.dumps({"log2_elems": E, "dictionary": args.dictionary, "pcg_K": K, "pcg_iters": args.pcg_iters, "ms_on": round(ms_on, 3),
                      "ms_off": round(ms_off, 3), "ms_per_col_on": round(ms_on / K, 3), "ms_per_col_off": round(ms_off / K, 3),
                      "ratio_on_off": round(ms_on / ms_off, 4), "spread_on": [round(min(t[True]), 3), round(max(t[True]), 3)],
                      "spread_off": [round(min(t[False]), 3), round(max(t[False]), 3)]}), flush=True)
    option(False)
    for v in (dB, dX):
        v.free()
    H.free()


if __name__ == "__main__":
    main()
