#!/usr/bin/env python3
"""Time of the V-cycle as a preconditioner applies it: vcycle_dev(None, b, x), no first iterate (pcg, fgmres and ldiv call
aggmg_vcycle_dev with x0 == NULL).  The flagship hierarchy of bench.py (DG p = 3, ratios 4:2:2, V(3,3)) and its timing
bracket: warm-up, synchronise, the loop, synchronise.  One JSON line.

    python tools/exp_zero_guess_cycle.py [--log2-elems 24] [--steps 20] [--warmup 5]

AGGMG_REPLAY_PRESMOOTH=0 in the environment gives the storing cycle of the same library (profiles/r28_replay.md)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-elems", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import uniform
    ctx = mg.Context(0)
    U = uniform.UniformDgAggHierarchy(2 ** args.log2_elems, p=3, pAgg=1, ratios=(4, 2, 2))
    H = uniform.build_device_hierarchy(U, ctx)
    b = ctx.to_device(U.rhs())
    x = ctx.alloc(len(U.rhs()))
    del U
    replays = getattr(ctx, "replay_launches", lambda: 0)   # (a library from before the option: 0)
    k0 = replays()

    def run(reps):
        for _ in range(reps):
            H.vcycle_dev(None, b, x)

    run(args.warmup)
    ctx.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"log2_elems": args.log2_elems, "steps": args.steps, "warmup": args.warmup,
                      "ms_per_cycle": 1e3 * dt / args.steps, "replayed_cycles": replays() - k0}))
    H.free()


if __name__ == "__main__":
    main()
