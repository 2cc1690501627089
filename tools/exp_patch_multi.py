#!/usr/bin/env python3
"""The K-column cycle on multiplicative patch levels (AGGMG_OPT_PATCH_MULTI) against the column-by-column cycle it
replaces, on DG p = 3 -> AggDG 4:1 -> 2:1 -> 2:1 with the multiplicative patch smoother on the fine level ("patchGS0")
or on every smoothed level ("patchGS"), zero initial guesses:

    python tools/exp_patch_multi.py --log2-elems 20 --smoother patchGS0 [--K 2 4 8] [--reps 9] [--dictionary 1]

--smoother patchSchwarz0 | patchSchwarz: the same for the hybrid patch smoother and its option, AGGMG_OPT_PATCH_SCHWARZ_MULTI
(DESIGN.md section 25); the Krylov line is then fgmres_multi to 1e-8 ||b|| on every K (the hybrid cycle is not symmetric:
no pcg), option on against off, alternating.  --group-width (hybrid smoothers): a group of eight columns as one launch of
eight against two launches of four per sweep launch (AGGMG_PATCH_SCHWARZ_MULTI_COLS, read when a context is created): two
contexts with a hierarchy each in this process, the V(3,3) cycle on N x 8 timed alternately.

One process per (size, smoother): run each under a time limit of its own.  Both sides are the SAME call,
vcycle_multi_dev V(3,3) on the same hierarchy and buffers, with the option on and off (it is read at every call); a
warm-up of both, then the two timed alternately, medians.  pcg on N x 8 (10 iterations, tolerance 0) the same way.
Per K one JSON line: ms per cycle and per column on either side, the ratio on / off, the patch sweep launches of one
cycle on the fine level on either side (HIP-event time, profiling on, a run of its own) and their compulsory bytes -- per launch
of kc columns the classes (2 B per element; without a dictionary the operator records, 8 (5 m^2 + 2 m) B per element
with compressed couplings) and 8 m B per element, column and vector (b, u in, u out; no u in from the zero iterate) --
over that time."""
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
    ap.add_argument("--smoother", default="patchGS0", choices=["patchGS0", "patchGS", "patchSchwarz0", "patchSchwarz"])
    ap.add_argument("--K", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dictionary", type=int, default=1)
    ap.add_argument("--pcg-iters", type=int, default=10)
    ap.add_argument("--group-width", action="store_true")
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib, uniform
    hybrid = args.smoother.startswith("patchSchwarz")
    if args.group_width:
        if not hybrid:
            ap.error("--group-width is about the hybrid smoothers' kernel")
        return group_width(args, mg, _lib, uniform)
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, args.dictionary)
    E = args.log2_elems
    U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
    H = uniform.build_device_hierarchy(U, ctx, smoother=args.smoother)
    N = H._ops[0].shape[0]
    ne, m = 2 ** E, N // 2 ** E
    Kmax = max(max(args.K), 8)
    rng = np.random.default_rng(E)
    dB = mg.DeviceMatrix(ctx, N, Kmax)
    dB.upload(np.asfortranarray(rng.standard_normal((N, Kmax))))
    dX = mg.DeviceMatrix(ctx, N, Kmax)
    zeros = np.zeros((N, Kmax), order="F")
    nclasses = H.mSmoothers[0].dictionary_classes

    def option(on):
        ctx.set_option(_lib.OPT_PATCH_SCHWARZ_MULTI if hybrid else _lib.OPT_PATCH_MULTI, 1 if on else 0)

    def counter():
        return ctx.patch_schwarz_multi_launches() if hybrid else ctx.patch_multi_launches()

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
        # the fine level's sweep launches of one cycle on either side: event time, in a run of its own
        sweeps_ms, sweeps_n, launches = {}, {}, 0
        for on in (True, False):
            option(on)
            ctx.synchronize()
            before = counter()
            ctx.profile_enable(1)
            for _ in range(args.reps):
                H.vcycle_multi_dev(None, dB, dX, K, N)
            st = ctx.profile_collect()
            ctx.profile_enable(False)
            if on:
                launches = (counter() - before) // args.reps
            s_ms, s_n = st.get(("smooth", 0), (0.0, 0))
            sweeps_ms[on], sweeps_n[on] = s_ms / args.reps, s_n // args.reps   # of one cycle: pre and post launches
        rec = 2 if nclasses else 8 * (5 * m * m + 2 * m)
        nbytes = 0
        for c0 in range(0, K, group):
            kc = min(group, K - c0)
            nbytes += (ne * rec + kc * N * 8 * 2) + (ne * rec + kc * N * 8 * 3)   # pre (zero iterate), post
        nbytes_off = K * ((ne * rec + N * 8 * 2) + (ne * rec + N * 8 * 3))   # column by column: the records once per column
        print(json.dumps({
            "log2_elems": E, "smoother": args.smoother, "dictionary_classes": nclasses, "K": K, "fused_on": fused, "group": group,
            "ms_on": round(ms_on, 4), "ms_off": round(ms_off, 4), "ms_per_col_on": round(ms_on / K, 4),
            "ms_per_col_off": round(ms_off / K, 4), "ratio_on_off": round(ms_on / ms_off, 4),
            "spread_on": [round(min(t[True]), 4), round(max(t[True]), 4)], "spread_off": [round(min(t[False]), 4), round(max(t[False]), 4)],
            "patch_multi_launches_per_cycle": int(launches), "fine_sweep_launches_on": int(sweeps_n[True]),
            "fine_sweep_launches_off": int(sweeps_n[False]), "fine_sweeps_ms_on": round(sweeps_ms[True], 4),
            "fine_sweeps_ms_off": round(sweeps_ms[False], 4), "fine_sweeps_bytes_on": int(nbytes), "fine_sweeps_bytes_off": int(nbytes_off),
            "fine_sweeps_TBps_on": round(nbytes / (sweeps_ms[True] * 1e-3) / 1e12, 4) if sweeps_ms[True] > 0 else None,
            "fine_sweeps_TBps_off": round(nbytes_off / (sweeps_ms[False] * 1e-3) / 1e12, 4) if sweeps_ms[False] > 0 else None}),
            flush=True)

    if hybrid:   # fgmres_multi to 1e-8 ||b|| from zero guesses, every K
        for K in args.K:
            its = {}

            def fgmres():
                its[0] = H.fgmres_multi_dev(dB, dX, K, N, 30, 200, 1e-8, 3, 3, 2.0 / 3.0)[0]

            t = {True: [], False: []}
            for rep in range(-1, args.reps):   # (rep -1: warm-up)
                for on in (True, False):
                    option(on)
                    dX.upload(zeros)
                    ms = timed(fgmres)
                    if rep >= 0:
                        t[on].append(ms)
            ms_on, ms_off = float(np.median(t[True])), float(np.median(t[False]))
            print(json.dumps({"log2_elems": E, "smoother": args.smoother, "dictionary_classes": nclasses, "fgmres_K": K,
                              "iters": [int(i) for i in its[0]], "ms_on": round(ms_on, 3), "ms_off": round(ms_off, 3),
                              "ratio_on_off": round(ms_on / ms_off, 4), "spread_on": [round(min(t[True]), 3), round(max(t[True]), 3)],
                              "spread_off": [round(min(t[False]), 3), round(max(t[False]), 3)]}), flush=True)
        option(False)
        for v in (dB, dX):
            v.free()
        H.free()
        return

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
    print(json.dumps({"log2_elems": E, "smoother": args.smoother, "pcg_K": K, "pcg_iters": args.pcg_iters, "ms_on": round(ms_on, 3),
                      "ms_off": round(ms_off, 3), "ms_per_col_on": round(ms_on / K, 3), "ms_per_col_off": round(ms_off / K, 3),
                      "ratio_on_off": round(ms_on / ms_off, 4)}), flush=True)
    option(False)
    for v in (dB, dX):
        v.free()
    H.free()


def group_width(args, mg, _lib, uniform):
    """V(3,3) on N x 8 with the option on: one launch of eight columns per sweep launch against two of four"""
    E, K = args.log2_elems, 8
    side = {}
    for cols in (8, 4):
        os.environ["AGGMG_PATCH_SCHWARZ_MULTI_COLS"] = str(cols)
        ctx = mg.Context(0)
        ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, args.dictionary)
        ctx.set_option(_lib.OPT_PATCH_SCHWARZ_MULTI, 1)
        U = uniform.UniformDgAggHierarchy(2 ** E, p=3, pAgg=1, ratios=(4, 2, 2))
        H = uniform.build_device_hierarchy(U, ctx, smoother=args.smoother)
        N = H._ops[0].shape[0]
        dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
        dB.upload(np.asfortranarray(np.random.default_rng(E).standard_normal((N, K))))
        side[cols] = (ctx, H, dB, dX, N)
    del os.environ["AGGMG_PATCH_SCHWARZ_MULTI_COLS"]
    t, launches = {8: [], 4: []}, {}
    for rep in range(-1, args.reps):   # (rep -1: warm-up)
        for cols in (8, 4):
            ctx, H, dB, dX, N = side[cols]
            before = ctx.patch_schwarz_multi_launches()
            ctx.synchronize()
            t0 = time.perf_counter()
            H.vcycle_multi_dev(None, dB, dX, K, N)
            ctx.synchronize()
            if rep >= 0:
                t[cols].append((time.perf_counter() - t0) * 1e3)
            launches[cols] = ctx.patch_schwarz_multi_launches() - before
    same = bool(np.array_equal(side[8][3].download().view(np.uint64), side[4][3].download().view(np.uint64)))
    print(json.dumps({"log2_elems": E, "smoother": args.smoother, "dictionary_classes": side[8][1].mSmoothers[0].dictionary_classes,
                      "K": K, "ms_one_launch_of_8": round(float(np.median(t[8])), 4), "ms_two_launches_of_4": round(float(np.median(t[4])), 4),
                      "spread_8": [round(min(t[8]), 4), round(max(t[8]), 4)], "spread_4": [round(min(t[4]), 4), round(max(t[4]), 4)],
                      "sweep_launches_per_cycle": {"8": int(launches[8]), "4": int(launches[4])}, "same_bits": same}), flush=True)


if __name__ == "__main__":
    main()
