"""Element-patch smoothers on the element-partitioned cycle, measured on ONE GPU.

  share   one rank's share of a W-rank job with device-local loop-back collectives (as tools/exp_dist_rank.py): ms per
          cycle -- HIP events on the library's stream, 3 warm-ups, median of 10 batches -- and dispatches per cycle
          (profiled launches + collectives), for block Jacobi, patchGS0 and patchGS, with the interface exchange of the
          next cycle under the split ascent (overlap 1) and after the plain ascent (overlap 0).
  solve   W ranks as THREADS of one process sharing the GPU (as tools/exp_dist_pcg.py): distributed.pcg and
          distributed.multigrid to tol ||b|| on block Jacobi, patchGS0 and patchGS: iterations, exchanges, time.
          A rehearsal of the code path, NOT a scaling measurement: the ranks share one GPU and every collective is a
          barrier between threads.

    python tools/exp_dist_patch.py share --log2-elems 22 24 [--world 8] [--rank 3]
    python tools/exp_dist_patch.py solve --log2-elems 20 [--world 8]
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

P, RATIOS, ALPHA = 3, (4, 2, 2), 2.0 / 3.0
SMOOTHERS = ("blockJac", "patchGS0", "patchGS")


def local_engine(mg, D, _lib, uniform, ctx, n, world, rank, smoother, nsw):
    """rank's local hierarchy with `smoother` and a replicated coarsest operator made of the uniform mesh's interior
    block row with the domain's end rows (no collective: what exp_dist_rank.py builds)"""
    kinds = D.smoother_kinds(smoother, len(RATIOS))
    layout = D.RankLayout(n, RATIOS, [P + 1, 2, 2, 2], world, rank, nsw, nsw, smoothers=None if smoother == "blockJac" else kinds)
    U = uniform.UniformDgAggHierarchy(n, p=P, pAgg=1, ratios=RATIOS, elem_range=layout.loc[0])
    nl = U.nlevels
    ops = [mg.DeviceOperator(U.stiffness_csc(k), _lib.OP_STIFFNESS, ctx) for k in range(nl)]
    sms = []
    for k in range(nl - 1):
        inds = U.descriptor(k).mBlockInds
        if kinds[k] == "patchGS":
            sms.append(mg.ElementPatchGaussSeidel(ops[k], inds.shape[0], inds.shape[1], ctx=ctx))
        else:
            sms.append(mg.BlockJacobi(ops[k], inds, ctx))
    Ls = [mg.DeviceOperator(U.interpolation_csc(k), _lib.OP_TRANSFER, ctx) for k in range(nl - 1)]
    H = mg.MeshHierarchy([U.descriptor(k) for k in range(nl)], ops, sms, Ls, ctx=ctx, keep_host=False,
                         coarse_mode=_lib.COARSE_EXTERNAL)
    nc, E = nl - 1, 16 * 8
    Ul = uniform.UniformDgAggHierarchy(n, p=P, pAgg=1, ratios=RATIOS, elem_range=(0, E))
    Ur = uniform.UniformDgAggHierarchy(n, p=P, pAgg=1, ratios=RATIOS, elem_range=(n - E, n))
    mid = [x[len(x) // 2] for x in U.levels[nc]['A']]
    g = [np.broadcast_to(b, (layout.ne[nc],) + b.shape).copy() for b in mid]
    for i in range(3):
        g[i][:4] = Ul.levels[nc]['A'][i][:4]
        g[i][-4:] = Ur.levels[nc]['A'][i][-4:]
    colptr, rowval, nzval, N = uniform.block_tridiag_to_csc(*g)
    Ac = mg.DeviceOperator(uniform._csc(colptr, rowval, nzval, (N, N)), _lib.OP_STIFFNESS, ctx)
    Hc = D._replicated_coarse_hierarchy(Ac, ctx, world)
    return D.HipEngine(H, Hc, ctx), layout, U


class NoComm:
    staged = False

    def __init__(self, world, rank):
        self.world, self.rank = world, rank


def share(args):
    import torch
    from agglomerationmultigrid1d_amd import _lib, uniform
    from agglomerationmultigrid1d_amd import api as mg
    from agglomerationmultigrid1d_amd import distributed as D
    nsw = 3
    for E in args.log2_elems:
        n = 2 ** E
        for smoother in SMOOTHERS:
            ctx = mg.Context(0)
            engine, layout, U = local_engine(mg, D, _lib, uniform, ctx, n, args.world, args.rank, smoother, nsw)
            dv = D.NativeDistributedVCycle(engine, layout, NoComm(args.world, args.rank), collectives="loopback")
            stream = torch.cuda.Stream()
            ctx.set_stream(stream.cuda_stream)        # the library's launches on a stream torch's events can bracket
            b = torch.from_numpy(U.rhs()).to(engine.dev)
            x, y = engine.new(layout.local_dofs(0)), engine.new(layout.local_dofs(0))
            torch.cuda.synchronize()
            for overlap in (0, 1):
                def batch(k):
                    nonlocal x, y
                    for _ in range(k):
                        dv.vcycle(x, b, y, nsw, nsw, ALPHA, overlap_next=bool(overlap))
                        x, y = y, x
                for _ in range(3):
                    batch(args.batch)
                ms = []
                for _ in range(10):
                    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    ctx.synchronize()
                    a.record(stream)
                    batch(args.batch)
                    z.record(stream)
                    z.synchronize()
                    ms.append(a.elapsed_time(z) / args.batch)
                ex0 = dv.exchanges
                ctx.profile_enable(1)
                batch(4)
                ctx.synchronize()
                ctx.profile_enable(0)
                launches = sum(v[1] for v in ctx.profile_collect().values()) / 4
                print(json.dumps({"what": "share", "log2_elems": E, "world": args.world, "rank": args.rank, "smoother": smoother,
                                  "overlap": overlap, "split_ascent": bool(overlap) and engine.H.can_split_up(nsw), "W": layout.W,
                                  "chunked": dv.chunked, "ms_per_cycle": round(float(np.median(ms)), 4),
                                  "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                                  "launches_per_cycle": launches, "collectives_per_cycle": (dv.exchanges - ex0) / 4,
                                  "dispatches_per_cycle": launches + (dv.exchanges - ex0) / 4}), flush=True)
            dv.free()
            engine.H.free()
            ctx.close()


def solve(args):
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    world = args.world
    for E in args.log2_elems:
        n = 2 ** E
        for smoother in SMOOTHERS:
            group = D.ThreadGroup(world)
            out, errs = [None] * world, []

            def rank_fn(rank):
                comm = D.ThreadComm(group, rank)
                ctx = mg.Context(0)
                kinds = D.smoother_kinds(smoother, len(RATIOS))
                layout = D.RankLayout(n, RATIOS, [P + 1, 2, 2, 2], world, rank, smoothers=None if smoother == "blockJac" else kinds)
                engine, U = D.build_local_uniform(n, P, 1, RATIOS, layout, ctx, comm, smoother=smoother)
                dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
                b = torch.from_numpy(U.rhs()).to(engine.dev)
                nloc = layout.local_dofs(0)

                def timed(fn):
                    torch.cuda.synchronize()
                    comm.barrier()
                    ex0, t0 = dv.exchanges, time.perf_counter()
                    r = fn()
                    torch.cuda.synchronize()
                    return r, comm.max(time.perf_counter() - t0), dv.exchanges - ex0

                D.pcg(dv, b, maxiter=2, tol=1e-30)                       # warm-up
                (_, it_p, res_p), t_p, ex_p = timed(lambda: D.pcg(dv, b, maxiter=300, tol=args.tol))
                (_, it_m, res_m), t_m, ex_m = timed(lambda: D.multigrid(dv, engine.new(nloc), b, 400, args.tol))
                comm.barrier()
                dv.free()
                return {"what": "solve", "log2_elems": E, "world": world, "smoother": smoother, "tol": args.tol, "W": layout.W,
                        "rehearsal": "ranks are threads sharing ONE GPU, host-staged collectives: not a scaling measurement",
                        "pcg": {"iterations": it_p, "exchanges": ex_p, "ms": round(1e3 * t_p, 2), "final_res": res_p[-1]},
                        "multigrid": {"cycles": it_m, "exchanges": ex_m, "ms": round(1e3 * t_m, 2), "final_res": res_m[-1]}}

            def one(r):
                try:
                    out[r] = rank_fn(r)
                except BaseException:
                    import traceback
                    errs.append(traceback.format_exc())
                    group.barrier.abort()

            # daemon threads joined against one deadline: a rank that hangs ends the tool instead of hanging it
            ts = [threading.Thread(target=one, args=(r,), daemon=True) for r in range(world)]
            deadline = time.monotonic() + args.limit
            for t in ts:
                t.start()
            for t in ts:
                t.join(max(0.0, deadline - time.monotonic()))
            if errs:
                sys.exit(errs[0])
            if any(t.is_alive() for t in ts):
                group.barrier.abort()
                sys.stderr.write(f"exp_dist_patch: a rank did not finish within {args.limit:g} s\n")
                sys.stderr.flush()
                os._exit(3)                  # (a rank stuck inside a library call would keep the interpreter from exiting)
            print(json.dumps(out[0]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("share", "solve"))
    ap.add_argument("--log2-elems", type=int, nargs="+", default=None)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=3)
    ap.add_argument("--batch", type=int, default=10, help="cycles per timed batch (share)")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds after which a solve whose ranks have not finished is ended")
    args = ap.parse_args()
    if args.log2_elems is None:
        args.log2_elems = [22, 24] if args.mode == "share" else [20]
    {"share": share, "solve": solve}[args.mode](args)


if __name__ == "__main__":
    main()
