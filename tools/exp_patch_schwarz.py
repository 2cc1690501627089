#!/usr/bin/env python3
"""Element-patch Schwarz smoother (aggmg_patch_schwarz_setup) on the config 3 hierarchy (DG p = 3 ->
AggDG 4:1 -> 2:1 -> 2:1) and on the ragged one (jittered mesh, agglomerates of different sizes):

    python tools/exp_patch_schwarz.py [--log2-elems 20 22] [--ragged-log2 20] [--reps 20] [--no-solve]
    python tools/exp_patch_schwarz.py --dictionary [--log2-elems 20 22] [--reps 10]

Times are HIP events on the context's stream (a torch stream the context is given), 3 warm-up calls, medians of --reps;
the variants of a comparison alternate in one process.

launch: the fused sweep launch on the fine level for S = 1, 3, 6 sweeps, its compulsory bytes
(aggmg_smoother_launch_bytes) and the fraction of 8 TB/s they make of the launch's time.

cycle: one V(3,3) cycle from a zero guess with, on level 0, the fused patch smoother, the generic route on the same lists
(HybridSchwarzSmoother; only up to --generic-max-log2 elements), block-Jacobi, and block-Jacobi with a Chebyshev
schedule.  GATE at 2^20 elements: fused <= 0.5 generic.

solve: time and iterations to 1e-8 ||b|| of multigrid V(3,3), fgmres V(1,1) and V(3,3) with the patch smoother, against
multigrid with block-Jacobi, with its Chebyshev schedule, and pcg with block-Jacobi.

--dictionary: the smoother's operator dictionary (AGGMG_OPT_OPERATOR_DICTIONARY) on / off -- two contexts with the option
on and two with it off in one process, on one stream, the four legs alternating inside every repetition: set-up time of
aggmg_patch_schwarz_setup (host clock around the synchronous call) and class counts, the sweep launch for S = 1, 3, 6 with
its compulsory bytes each way, one V(3,3) cycle, the multigrid and fgmres V(3,3) solves.  The second off leg runs the
same kernels as the first: the spread between the two is the noise margin beside every on / off ratio.  GATE at 2^22
elements, S = 3: on <= off (within that margin).  One JSON line per measurement.

--gs: the multiplicative two-colour smoother (aggmg_patch_gs_setup) against the hybrid one, for the
operator dictionary on and then off: contexts "hybrid", "hybrid2" (patchSchwarz0 twice: the spread of the two is the noise
margin), "gs0" (patchGS0) and "gs" (patchGS on every smoothed level) on one stream, alternating inside every repetition.
The sweep launch for S = 1, 3, 6, one V(3,3) cycle, and the solves to 1e-8 ||b||: multigrid V(3,3) and V(2,2) on the hybrid
legs and on gs0, fgmres V(3,3) on the hybrid leg, pcg V(3,3), V(2,2), V(1,1) on gs0 and gs.  CONDITION at 2^20 elements with
the dictionary on: multigrid V(3,3) on gs0 takes no longer than on hybrid, by more than that margin."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, nargs="*", default=[20, 22])
    ap.add_argument("--ragged-log2", type=int, nargs="*", default=[20])
    ap.add_argument("--generic-max-log2", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-solve", action="store_true")
    ap.add_argument("--dictionary", action="store_true")
    ap.add_argument("--gs", action="store_true")
    args = ap.parse_args()
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import _lib, uniform
    ctx = mg.Context(0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    if args.dictionary or args.gs:
        (dictionary_legs if args.dictionary else gs_legs)(args, torch, mg, _lib, uniform, stream)
        ctx.close()
        return
    lib, h = ctx.lib, ctx.handle
    pd = ctypes.POINTER(ctypes.c_double)

    def timed_all(fns, reps=None, warm=3):
        """median ms of every fn of the dict, the fns alternating inside every repetition"""
        for _ in range(warm):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(reps or args.reps):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ctx.synchronize()
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        return {k: float(np.median(v)) for k, v in ms.items()}

    def launches(tag, E, op, S, m, ne):
        N = op.shape[0]
        rng = np.random.default_rng(E)
        du, db, dout = ctx.to_device(rng.standard_normal(N)), ctx.to_device(rng.standard_normal(N)), ctx.alloc(N)
        rd, wr = mg.smoother_launch_bytes(op, S, "sweeps")
        t = timed_all({s: (lambda s=s: ctx.check(lib.aggmg_smooth_dev(h, op.handle, S.handle, du.ptr, db.ptr, 2.0 / 3.0, s, dout.ptr)))
                       for s in (1, 3, 6)})
        for s, ms in t.items():
            print(json.dumps({"what": "launch", "hierarchy": tag, "log2_elems": E, "m": m, "sweeps": s, "ms": round(ms, 4),
                              "bytes": rd + wr, "bytes_per_element": round((rd + wr) / ne, 1),
                              "of_8TBs": round((rd + wr) / (ms * 1e-3) / PEAK, 3)}), flush=True)
        for v in (du, db, dout):
            v.free()

    for E in args.log2_elems:
        ne = 2 ** E
        U = uniform.UniformDgAggHierarchy(ne, p=3, pAgg=1, ratios=(4, 2, 2))
        csc = ([U.stiffness_csc(k) for k in range(U.nlevels)], [U.interpolation_csc(k) for k in range(U.nlevels - 1)])
        b = U.rhs()
        nb = float(np.linalg.norm(b))
        Hs = {"patch": uniform.build_device_hierarchy(U, ctx, smoother="patchSchwarz0", csc=csc),
              "blockjac": uniform.build_device_hierarchy(U, ctx, csc=csc),
              "blockjac_cheb": uniform.build_device_hierarchy(U, ctx, csc=csc)}
        lam = Hs["blockjac_cheb"].estimate_lambda_max(0)
        Hs["blockjac_cheb"].set_sweep_weights(0, mg.chebyshev_weights(lam, degree=3), mg.chebyshev_weights(lam, degree=3)[::-1])
        if E <= args.generic_max_log2:   # the generic route on the same lists: level 0 only, block-Jacobi below
            ops = [mg.DeviceOperator(csc[0][k], _lib.OP_STIFFNESS, ctx) for k in range(U.nlevels)]
            sms = [mg.HybridSchwarzSmoother(ops[0], mg.element_patch_lists(4, ne), ctx)]
            sms += [mg.BlockJacobi(ops[k], U.descriptor(k).mBlockInds, ctx) for k in range(1, U.nlevels - 1)]
            Ls = [mg.DeviceOperator(csc[1][k], _lib.OP_TRANSFER, ctx) for k in range(U.nlevels - 1)]
            Hs["generic"] = mg.MeshHierarchy([U.descriptor(k) for k in range(U.nlevels)], ops, sms, Ls, ctx=ctx, keep_host=False)
        assert Hs["patch"].mSmoothers[0].fused and Hs["patch"].level_kinds()[0] == "fused_btd"
        launches("config3", E, Hs["patch"]._ops[0], Hs["patch"].mSmoothers[0], 4, ne)
        N = len(b)
        db, dx, zero = ctx.to_device(b), ctx.alloc(N), ctx.alloc(N)
        t = timed_all({k: (lambda H=H: H.vcycle_dev(None, db, dx, 3, 3)) for k, H in Hs.items()})
        row = {"what": "cycle", "log2_elems": E, "cycle": "V(3,3)", "ms": {k: round(v, 4) for k, v in t.items()}}
        if "generic" in t:
            row["fused_over_generic"] = round(t["patch"] / t["generic"], 4)
            row["gate_fused_at_most_half_of_generic"] = bool(t["patch"] <= 0.5 * t["generic"])
        print(json.dumps(row), flush=True)
        if not args.no_solve:
            hist = np.zeros(400)
            it, nchk = ctypes.c_int(0), ctypes.c_int(0)

            def solve(H, kind, nPre, nPost):
                def run():
                    ctx.check(lib.aggmg_copy_segments_dev(h, 1, (ctypes.c_void_p * 1)(zero.ptr.value),
                                                          (ctypes.c_void_p * 1)(dx.ptr.value), (ctypes.c_int64 * 1)(1),
                                                          (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N)))
                    if kind == "multigrid":
                        ctx.check(lib.aggmg_multigrid_dev(h, H.handle, zero.ptr, db.ptr, 400, 1e-8, 1, nPre, nPost, 2.0 / 3.0,
                                                          dx.ptr, hist.ctypes.data_as(pd), ctypes.byref(it), ctypes.byref(nchk),
                                                          None, None))
                    elif kind == "pcg":
                        ctx.check(lib.aggmg_pcg_dev(h, H.handle, db.ptr, dx.ptr, 400, 1e-8, nPre, nPost, 2.0 / 3.0,
                                                    hist.ctypes.data_as(pd), ctypes.byref(it)))
                    else:
                        ctx.check(lib.aggmg_fgmres_dev(h, H.handle, db.ptr, dx.ptr, 30, 400, 1e-8, nPre, nPost, 2.0 / 3.0,
                                                       hist.ctypes.data_as(pd), ctypes.byref(it)))
                return run

            for name, kind, nPre, nPost in (("patch", "multigrid", 3, 3), ("patch", "fgmres", 1, 1), ("patch", "fgmres", 3, 3),
                                            ("blockjac", "multigrid", 3, 3), ("blockjac_cheb", "multigrid", 3, 3),
                                            ("blockjac", "pcg", 3, 3)):
                ms = timed_all({"s": solve(Hs[name], kind, nPre, nPost)}, reps=max(3, args.reps // 4), warm=1)["s"]
                true = float(np.linalg.norm(mg.residual(Hs[name]._ops[0], dx.download(), b))) if E <= 22 else None
                print(json.dumps({"what": "solve", "log2_elems": E, "level0": name, "solver": kind, "cycle": f"V({nPre},{nPost})",
                                  "iterations": it.value, "ms": round(ms, 3),
                                  "true_residual_over_b": None if true is None else true / nb}), flush=True)
        for v in (db, dx, zero):
            v.free()
        for H in Hs.values():
            H.free()
        del Hs

    for E in args.ragged_log2:
        ne = 2 ** E
        H, b, _ = uniform.build_device_ragged_hierarchy(ne, ctx)
        op = H._ops[0]
        S = mg.ElementPatchSchwarz(op, 4, ne, ctx=ctx)
        assert S.fused
        launches("ragged", E, op, S, 4, ne)
        S.free()
        H.free()
    ctx.close()


def dictionary_legs(args, torch, mg, _lib, uniform, stream):
    import time
    pd = ctypes.POINTER(ctypes.c_double)
    legs = {"on": 1, "off": 0, "on2": 1, "off2": 0}
    ctxs = {}
    for name, v in legs.items():
        ctxs[name] = mg.Context(0)
        ctxs[name].set_stream(stream.cuda_stream)
        ctxs[name].set_option(_lib.OPT_OPERATOR_DICTIONARY, v)

    def timed_all(fns, reps, warm=3):
        for _ in range(warm):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        return {k: float(np.median(v)) for k, v in ms.items()}

    def ratios(t):
        """on / off and, beside it, the spread of the two legs that run the same kernels"""
        return {"on_over_off": round(t["on"] / t["off"], 4), "on2_over_off2": round(t["on2"] / t["off2"], 4),
                "off2_over_off": round(t["off2"] / t["off"], 4), "on2_over_on": round(t["on2"] / t["on"], 4)}

    for E in args.log2_elems:
        ne = 2 ** E
        U = uniform.UniformDgAggHierarchy(ne, p=3, pAgg=1, ratios=(4, 2, 2))
        csc = ([U.stiffness_csc(k) for k in range(U.nlevels)], [U.interpolation_csc(k) for k in range(U.nlevels - 1)])
        b = U.rhs()
        N = len(b)
        # set-up of the smoother alone, on an operator of its own per leg: 1 warm-up + 3 timed, legs alternating
        setup = {k: [] for k in legs}
        for r in range(4):
            for name, c in ctxs.items():
                op = mg.DeviceOperator(csc[0][0], _lib.OP_STIFFNESS, c)
                c.synchronize()
                t0 = time.perf_counter()
                S = mg.ElementPatchSchwarz(op, 4, ne, ctx=c)
                c.synchronize()
                if r:
                    setup[name].append((time.perf_counter() - t0) * 1e3)
                S.free()
                op.free()
        print(json.dumps({"what": "setup", "log2_elems": E, "ms": {k: round(float(np.median(v)), 2) for k, v in setup.items()}}),
              flush=True)
        Hs = {k: uniform.build_device_hierarchy(U, c, smoother="patchSchwarz0", csc=csc) for k, c in ctxs.items()}
        print(json.dumps({"what": "classes", "log2_elems": E,
                          "patch": {k: H.patch_dictionary_levels() for k, H in Hs.items()},
                          "level": {k: H.dictionary_levels() for k, H in Hs.items()}}), flush=True)
        rng = np.random.default_rng(E)
        u0, rhs = rng.standard_normal(N), rng.standard_normal(N)
        vec = {k: (c.to_device(u0), c.to_device(rhs), c.alloc(N), c.to_device(b), c.alloc(N), c.alloc(N)) for k, c in ctxs.items()}
        by = {k: sum(mg.smoother_launch_bytes(H._ops[0], H.mSmoothers[0], "sweeps")) for k, H in Hs.items()}
        for s in (1, 3, 6):
            def launch(k, s=s):
                c, H = ctxs[k], Hs[k]
                du, dr, dout = vec[k][:3]
                return lambda: c.check(c.lib.aggmg_smooth_dev(c.handle, H._ops[0].handle, H.mSmoothers[0].handle, du.ptr, dr.ptr,
                                                              2.0 / 3.0, s, dout.ptr))
            t = timed_all({k: launch(k) for k in legs}, args.reps)
            row = {"what": "launch", "log2_elems": E, "sweeps": s, "ms": {k: round(v, 4) for k, v in t.items()},
                   "bytes_per_element": {k: round(by[k] / ne, 1) for k in legs},
                   "of_8TBs": {k: round(by[k] / (t[k] * 1e-3) / PEAK, 3) for k in legs}}
            row.update(ratios(t))
            if E == 22 and s == 3:
                margin = abs(t["off2"] / t["off"] - 1.0)
                row["gate_margin"] = round(margin, 4)
                row["gate_on_not_slower_than_off"] = bool(t["on"] <= t["off"] * (1.0 + margin))
            print(json.dumps(row), flush=True)
        t = timed_all({k: (lambda k=k: Hs[k].vcycle_dev(None, vec[k][3], vec[k][4], 3, 3)) for k in legs}, args.reps)
        row = {"what": "cycle", "log2_elems": E, "cycle": "V(3,3)", "ms": {k: round(v, 4) for k, v in t.items()}}
        row.update(ratios(t))
        print(json.dumps(row), flush=True)
        if not args.no_solve:
            hist = np.zeros(400)
            its = {k: ctypes.c_int(0) for k in legs}
            nchk = ctypes.c_int(0)

            def solve(k, kind):
                c, H = ctxs[k], Hs[k]
                db, dx, zero = vec[k][3:]

                def run():
                    c.check(c.lib.aggmg_copy_segments_dev(c.handle, 1, (ctypes.c_void_p * 1)(zero.ptr.value),
                                                          (ctypes.c_void_p * 1)(dx.ptr.value), (ctypes.c_int64 * 1)(1),
                                                          (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N)))
                    if kind == "multigrid":
                        c.check(c.lib.aggmg_multigrid_dev(c.handle, H.handle, zero.ptr, db.ptr, 400, 1e-8, 1, 3, 3, 2.0 / 3.0,
                                                          dx.ptr, hist.ctypes.data_as(pd), ctypes.byref(its[k]), ctypes.byref(nchk),
                                                          None, None))
                    else:
                        c.check(c.lib.aggmg_fgmres_dev(c.handle, H.handle, db.ptr, dx.ptr, 30, 400, 1e-8, 3, 3, 2.0 / 3.0,
                                                       hist.ctypes.data_as(pd), ctypes.byref(its[k])))
                return run

            for kind in ("multigrid", "fgmres"):
                t = timed_all({k: solve(k, kind) for k in legs}, max(3, args.reps // 3), warm=1)
                row = {"what": "solve", "log2_elems": E, "solver": kind, "cycle": "V(3,3)",
                       "iterations": {k: its[k].value for k in legs}, "ms": {k: round(v, 3) for k, v in t.items()}}
                row.update(ratios(t))
                print(json.dumps(row), flush=True)
        for vs in vec.values():
            for v in vs:
                v.free()
        for H in Hs.values():
            sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
            H.free()
            for x in sms + ops + Ls:
                x.free()
        del Hs
    for c in ctxs.values():
        c.close()


def gs_legs(args, torch, mg, _lib, uniform, stream):
    pd = ctypes.POINTER(ctypes.c_double)
    smoothers = {"hybrid": "patchSchwarz0", "hybrid2": "patchSchwarz0", "gs0": "patchGS0", "gs": "patchGS"}

    def timed_all(fns, reps, warm=3):
        for _ in range(warm):
            for fn in fns.values():
                fn()
        ms = {k: [] for k in fns}
        for _ in range(reps):
            for k, fn in fns.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record(stream)
                fn()
                b.record(stream)
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        return {k: float(np.median(v)) for k, v in ms.items()}

    def rounded(t):
        return {k: round(v, 4) for k, v in t.items()}

    for E in args.log2_elems:
        ne = 2 ** E
        U = uniform.UniformDgAggHierarchy(ne, p=3, pAgg=1, ratios=(4, 2, 2))
        csc = ([U.stiffness_csc(k) for k in range(U.nlevels)], [U.interpolation_csc(k) for k in range(U.nlevels - 1)])
        b = U.rhs()
        nb = float(np.linalg.norm(b))
        N = len(b)
        for dictionary in (1, 0):
            ctxs = {}
            for name in smoothers:
                ctxs[name] = mg.Context(0)
                ctxs[name].set_stream(stream.cuda_stream)
                ctxs[name].set_option(_lib.OPT_OPERATOR_DICTIONARY, dictionary)
            Hs = {k: uniform.build_device_hierarchy(U, c, smoother=smoothers[k], csc=csc) for k, c in ctxs.items()}
            tag = {"log2_elems": E, "dictionary": dictionary}
            print(json.dumps(dict(tag, what="classes", patch={k: H.patch_dictionary_levels() for k, H in Hs.items()})), flush=True)
            rng = np.random.default_rng(E)
            u0, rhs = rng.standard_normal(N), rng.standard_normal(N)
            vec = {k: (c.to_device(u0), c.to_device(rhs), c.alloc(N), c.to_device(b), c.alloc(N), c.alloc(N)) for k, c in ctxs.items()}
            three = ("hybrid", "hybrid2", "gs0")
            for s in (1, 3, 6):
                def launch(k, s=s):
                    c, H = ctxs[k], Hs[k]
                    du, dr, dout = vec[k][:3]
                    return lambda: c.check(c.lib.aggmg_smooth_dev(c.handle, H._ops[0].handle, H.mSmoothers[0].handle, du.ptr, dr.ptr,
                                                                  2.0 / 3.0, s, dout.ptr))
                t = timed_all({k: launch(k) for k in three}, args.reps)
                print(json.dumps(dict(tag, what="launch", sweeps=s, ms=rounded(t), gs0_over_hybrid=round(t["gs0"] / t["hybrid"], 4),
                                      hybrid2_over_hybrid=round(t["hybrid2"] / t["hybrid"], 4))), flush=True)
            t = timed_all({k: (lambda k=k: Hs[k].vcycle_dev(None, vec[k][3], vec[k][4], 3, 3)) for k in three}, args.reps)
            print(json.dumps(dict(tag, what="cycle", cycle="V(3,3)", ms=rounded(t), gs0_over_hybrid=round(t["gs0"] / t["hybrid"], 4),
                                  hybrid2_over_hybrid=round(t["hybrid2"] / t["hybrid"], 4))), flush=True)
            if not args.no_solve:
                hist = np.zeros(400)
                its = {k: ctypes.c_int(0) for k in smoothers}
                nchk = ctypes.c_int(0)

                def solve(k, kind, n):
                    c, H = ctxs[k], Hs[k]
                    db, dx, zero = vec[k][3:]

                    def run():
                        c.check(c.lib.aggmg_copy_segments_dev(c.handle, 1, (ctypes.c_void_p * 1)(zero.ptr.value),
                                                              (ctypes.c_void_p * 1)(dx.ptr.value), (ctypes.c_int64 * 1)(1),
                                                              (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N), (ctypes.c_int64 * 1)(N)))
                        if kind == "multigrid":
                            c.check(c.lib.aggmg_multigrid_dev(c.handle, H.handle, zero.ptr, db.ptr, 400, 1e-8, 1, n, n, 2.0 / 3.0,
                                                              dx.ptr, hist.ctypes.data_as(pd), ctypes.byref(its[k]), ctypes.byref(nchk),
                                                              None, None))
                        elif kind == "pcg":
                            c.check(c.lib.aggmg_pcg_dev(c.handle, H.handle, db.ptr, dx.ptr, 400, 1e-8, n, n, 2.0 / 3.0,
                                                        hist.ctypes.data_as(pd), ctypes.byref(its[k])))
                        else:
                            c.check(c.lib.aggmg_fgmres_dev(c.handle, H.handle, db.ptr, dx.ptr, 30, 400, 1e-8, n, n, 2.0 / 3.0,
                                                           hist.ctypes.data_as(pd), ctypes.byref(its[k])))
                    return run

                for kind, n, names in (("multigrid", 3, three), ("multigrid", 2, three), ("fgmres", 3, ("hybrid", "hybrid2")),
                                       ("pcg", 3, ("gs0", "gs")), ("pcg", 2, ("gs0", "gs")), ("pcg", 1, ("gs0", "gs"))):
                    t = timed_all({k: solve(k, kind, n) for k in names}, max(3, args.reps // 3), warm=1)
                    row = dict(tag, what="solve", solver=kind, cycle=f"V({n},{n})", iterations={k: its[k].value for k in names},
                               ms=rounded(t))
                    if E <= 22:
                        row["true_residual_over_b"] = {
                            k: float(np.linalg.norm(mg.residual(Hs[k]._ops[0], vec[k][4].download(), b))) / nb for k in names}
                    if kind == "multigrid":
                        margin = abs(t["hybrid2"] / t["hybrid"] - 1.0)
                        row["gs0_over_hybrid"] = round(t["gs0"] / t["hybrid"], 4)
                        row["margin"] = round(margin, 4)
                        if n == 3 and E == 20 and dictionary:
                            row["condition_gs0_no_slower_than_hybrid"] = bool(t["gs0"] <= t["hybrid"] * (1.0 + margin))
                    print(json.dumps(row), flush=True)
            for vs in vec.values():
                for v in vs:
                    v.free()
            for H in Hs.values():
                sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
                H.free()
                for x in sms + ops + Ls:
                    x.free()
            del Hs
            for c in ctxs.values():
                c.close()


if __name__ == "__main__":
    main()
