"""Conjugate gradients against the stationary loop on the element-partitioned path (distributed.pcg / distributed.multigrid),
config 4 on 8 ranks run as THREADS of one process sharing one GPU (ThreadGroup / ThreadComm, host-staged collectives, as
bench.py --rehearse-threads): milliseconds per PCG iteration beside milliseconds per partitioned cycle, and iterations
and time to ||r|| < 1e-8 ||b|| for both solvers in the same process.  A rehearsal of the 8-rank code path, not a
multi-GPU measurement: the ranks share the GPU and every collective is a barrier between threads.

    python tools/exp_dist_pcg.py [--log2-elems 20] [--world 8] [--cycles 20] [--limit 600] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=20)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--cycles", type=int, default=20, help="timed cycles / PCG iterations of the per-step figures")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--limit", type=float, default=600.0, help="seconds after which a run whose ranks have not finished is ended")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    world, n, p, ratios = args.world, 2 ** args.log2_elems, 3, (4, 2, 2)
    group = D.ThreadGroup(world)
    out, errs = [None] * world, []

    def rank_fn(rank):
        comm = D.ThreadComm(group, rank)
        ctx = mg.Context(0)
        layout = D.RankLayout(n, ratios, [p + 1, 2, 2, 2], world, rank)
        engine, U = D.build_local_uniform(n, p, 1, ratios, layout, ctx, comm)
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        nloc = layout.local_dofs(0)

        def timed(fn):
            torch.cuda.synchronize()
            comm.barrier()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, comm.max(time.perf_counter() - t0)

        def cycles(k):
            x, y = engine.new(nloc), engine.new(nloc)
            torch.cuda.synchronize()
            for _ in range(k):
                dv.vcycle(x, b, y, overlap_next=True)
                x, y = y, x

        cycles(3)                                                        # warm-up
        D.pcg(dv, b, maxiter=2, tol=1e-30)
        _, t_cyc = timed(lambda: cycles(args.cycles))
        # (tol 1e-30: exactly --cycles iterations; includes the one cycle and the norms in front of the loop)
        (_, it_fix, _), t_it = timed(lambda: D.pcg(dv, b, maxiter=args.cycles, tol=1e-30))
        (_, it_p, res_p), t_p = timed(lambda: D.pcg(dv, b, maxiter=200, tol=args.tol))
        (_, it_m, res_m), t_m = timed(lambda: D.multigrid(dv, engine.new(nloc), b, 400, args.tol))
        (_, it_m4, res_m4), t_m4 = timed(lambda: D.multigrid(dv, engine.new(nloc), b, 400, args.tol, check_every=4))
        comm.barrier()
        dv.free()
        return {
            "workload": f"config 4: DG p=3 n=2^{args.log2_elems} -> AggDG 4:1 -> 2:1 -> 2:1, V(3,3), {world} thread ranks on one GPU",
            "rehearsal": "ranks are threads sharing ONE GPU, host-staged collectives: not a multi-GPU measurement",
            "ms_per_partitioned_cycle": 1e3 * t_cyc / args.cycles,
            "ms_per_pcg_iteration": 1e3 * t_it / max(it_fix, 1),
            "tol": args.tol,
            "pcg": {"iterations": it_p, "ms": 1e3 * t_p, "final_res": res_p[-1]},
            "multigrid": {"cycles": it_m, "ms": 1e3 * t_m, "final_res": res_m[-1]},
            "multigrid_check_every_4": {"cycles": it_m4, "ms": 1e3 * t_m4, "final_res": res_m4[-1]},
        }

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
        sys.stdout.flush()
        sys.stderr.write(f"exp_dist_pcg: a rank did not finish within {args.limit:g} s\n")
        sys.stderr.flush()
        os._exit(3)                      # (a rank stuck inside a library call would keep the interpreter from exiting)
    line = json.dumps(out[0])
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
