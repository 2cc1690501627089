"""The element-partitioned V-cycle on the GPU -- distributed.py, csrc/dist.hip and the entry points they drive
(aggmg_vcycle_down_dev, aggmg_vcycle_up_split_dev, aggmg_vcycle_up_coarse_dev, aggmg_coarse_chunk_*, the owned-range
Krylov kernels) -- on meshes whose elements are unequal: the jittered meshes of jitter_helpers (every element's record
its own) and the periodic ones of periodic_helpers (few classes, neighbours always in different ones).  Every rank's
operators are slices of ONE global oracle hierarchy (dist_nonuniform_helpers), so an operator, inverse block or transfer
read at the wrong element offset -- a rank's offset, a tile subset of the split ascent, a block range of the chunked
coarsest solve, the rank order of the gathered coarsest block rows -- moves the result by the size of the iterate
(tests/test_distributed_nonuniform_cpu.py: 0.12 .. 3.0 of its norm; on the uniform meshes of every other partitioned
test: 1e-11).

Three assertions per case, after each of three cycles that feed their output back, from the first iterate
splitmix_normal(N, X0_SEED) whose ghosts are overwritten on every rank:
 1. the single-GPU cycle of the whole-range hierarchy (the same construction with a one-rank layout) against the oracle:
    ||A (x - x_ref)|| <= RESIDUAL_TOL (||b|| + ||A x_in||) and ||x - x_ref|| <= tol ||x_ref||, tol = jitter_helpers.ITERATE_TOL /
    periodic_helpers.ONE_CYCLE_ITERATE_TOL after the first cycle, loop_iterate_tol(cycle) after the later ones;
 2. the gathered owned slices of the partitioned run against the oracle: the same two bounds;
 3. the gathered owned slices == the single-GPU result as 64-bit patterns, wherever the uniform tests
    (test_distributed_gpu.py, test_gpu_dist_patch.py) assert err == 0.0.
Which form of the operator a rank reads depends on its local record count: c34_small, c34 on 4 and 8 ranks and the
periodic cases are within a dictionary's 1024 records on every local level; test_fine_level_over_the_dictionary_cap
(c34 on 2 ranks) runs the plain per-element arrays on the fine level.
The element-patch smoothers have no oracle cycle here: they go against the single-GPU hierarchy only (their sweeps are
held to their models in test_gpu_patch_schwarz.py / test_gpu_patch_gs.py).

Measured on an MI355X: assertion 3 holds as bits in every case that asserts it (partitioned and single-GPU figures are
therefore the same); against the oracle at most 2.0e-15 of the scale in the residual and 2.3e-10 in the iterate (c34,
second cycle; first cycles at most 3.2e-11).  The chunked coarsest solve differs from the single-GPU iterate, which
plans another solve, by 3.1e-10.

Every multi-rank step runs on threads joined under a time limit; after a device failure or a time limit nothing more
of this module starts (`_fault`)."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the process then holds one HIP runtime, torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")) if p not in sys.path]

import dist_nonuniform_helpers as nh      # noqa: E402
import jitter_helpers as jh               # noqa: E402
import periodic_helpers as ph             # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ALPHA, NCYC = jh.ALPHA, 3
_fault = []          # why nothing more may start on the GPU from this module


def _guard():
    if _fault:
        pytest.fail(f"not started: an earlier GPU step of this module failed ({_fault[0]})")


def _thread_ranks(world, fn, limit=240):
    """dist_nonuniform_helpers.thread_ranks (one library context per rank) under this module's `_fault` guard"""
    _guard()
    return nh.thread_ranks(world, fn, limit, fault=_fault, device_errors=("HIP error", "hipError", "illegal memory"))


shape_of = nh.shape_of


def iterate_tol(case, cycle):
    if case in ph.CASES:
        return ph.ONE_CYCLE_ITERATE_TOL if cycle == 1 else ph.loop_iterate_tol(cycle)
    return jh.ITERATE_TOL if cycle == 1 else jh.loop_iterate_tol(cycle)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


class _World:
    """oracle hierarchies and cycles (once per case), whole-range device hierarchies and their cycles (once per case
    and smoother); nothing of them is changed after it is made"""

    def __init__(self, oracle, mg):
        self.o, self.mg = oracle, mg
        self.hiers, self.cycles, self.single_h, self.single_x = {}, {}, {}, {}
        self.ctx = None

    def ref(self, case):
        if case not in self.hiers:
            Ho, b = nh.build(self.o, case, True)
            x0 = self.o.splitmix_normal(len(b), jh.X0_SEED)
            for v in (b, x0):
                v.setflags(write=False)
            self.hiers[case] = dict(Ho=Ho, b=b, x0=x0, A=Ho.mStiffness[0].tocsr(), N=len(b))
        return self.hiers[case]

    def oracle_cycles(self, case, sweeps=(3, 3), gs=False):
        """[x_1, x_2, x_3]: the oracle's cycle fed back three times from x0 (gs: its red-black block Gauss-Seidel
        restatement on the same blocks, as tests/test_gpu_blockgs.py)"""
        key = (case, sweeps, gs)
        if key not in self.cycles:
            r = self.ref(case)
            Ho = r["Ho"]
            if gs:
                Ho = copy.copy(Ho)
                Ho.mSmoothers = [self.o.BlockGaussSeidelRB(S.mBlocks, S.mBlockInds) for S in r["Ho"].mSmoothers]
            xs, x = [], r["x0"]
            for _ in range(NCYC):
                x = self.o.multigrid_v_cycle(Ho, x, r["b"], nPre=sweeps[0], nPost=sweeps[1], alpha=ALPHA)
                x.setflags(write=False)
                xs.append(x)
            self.cycles[key] = xs
        return self.cycles[key]

    def single(self, case, smoother="blockJac"):
        """the whole-range hierarchy: dist_nonuniform_helpers.build_local_engine with a one-rank layout"""
        from agglomerationmultigrid1d_amd import distributed as D
        key = (case, smoother)
        if key not in self.single_h:
            if self.ctx is None:
                self.ctx = self.mg.Context(0)
            n, ratios, ms = shape_of(case)
            kinds = D.smoother_kinds(smoother, len(ratios))
            layout = D.RankLayout(n, ratios, ms, 1, 0, 3, 3, gs=(smoother == "blockGS"), smoothers=kinds)
            H = nh.build_local_engine(self.mg, D, self.ref(case)["Ho"], layout, self.ctx, None, smoother)
            assert all(H.structured_levels()) and H.coarse_info()['on_device']
            self.single_h[key] = H
        return self.single_h[key]

    def single_cycles(self, case, smoother="blockJac", sweeps=(3, 3)):
        """[x_1, x_2, x_3] of the whole-range hierarchy from x0 -- held to the oracle (assertion 1) when they are made,
        so that whichever test asks for them first has checked them (the element-patch smoothers have no oracle cycle)"""
        key = (case, smoother, sweeps)
        if key not in self.single_x:
            r, H = self.ref(case), self.single(case, smoother)
            ctx = H.ctx
            bd = ctx.to_device(np.array(r["b"]))
            xa, xb = ctx.to_device(np.array(r["x0"])), ctx.alloc(r["N"])
            xs = []
            for _ in range(NCYC):
                H.vcycle_dev(xa, bd, xb, sweeps[0], sweeps[1], ALPHA)
                xa, xb = xb, xa
                x = xa.download()
                x.setflags(write=False)
                xs.append(x)
            if smoother in ("blockJac", "blockGS"):
                _against_the_oracle(r, case, xs, self.oracle_cycles(case, sweeps, gs=(smoother == "blockGS")),
                                    f"single GPU {smoother} {case} V{sweeps}")
            self.single_x[key] = xs
        return self.single_x[key]

    def close(self):
        for H in self.single_h.values():
            H.free()


@pytest.fixture(scope="module")
def world(oracle, mg):
    w = _World(oracle, mg)
    yield w
    w.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _against_the_oracle(r, case, xs, xrs, what):
    """assertions 1 / 2: after every cycle, ||A (x - x_ref)|| <= RESIDUAL_TOL (||b|| + ||A x_in||), x_in the reference's
    iterate that went into the cycle, and ||x - x_ref|| <= iterate_tol(case, cycle) ||x_ref||; figures printed first"""
    xin = r["x0"]
    for c, (x, xr) in enumerate(zip(xs, xrs), 1):
        scale = jh.cycle_scale(r["Ho"], r["b"], xin)
        res = float(np.linalg.norm(r["A"] @ (x - xr))) / scale
        rel = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
        print(f"[dist-nonuniform] {what} cycle {c}: ||A (x - x_ref)|| / scale = {res:.3e}   ||x - x_ref|| / ||x_ref|| = {rel:.3e} "
              f"(bound {iterate_tol(case, c):.1e})")
        assert np.all(np.isfinite(x)), (what, c)
        assert res <= jh.RESIDUAL_TOL, (what, c, res)
        assert rel <= iterate_tol(case, c), (what, c, rel)
        xin = xr


def _partitioned(mg, r, case, nranks, smoother="blockJac", sweeps=(3, 3), schedule="native", facts=None):
    """three partitioned cycles on thread ranks from the poisoned-ghost first iterate -> ([x_1, x_2, x_3] gathered from
    the owned slices, facts by rank); `facts(engine, layout, dv)` adds to a rank's facts.  can_split: the library's
    predicate for the hierarchy (MeshHierarchy.can_split_up), which its own schedule follows under overlap_next;
    split_taken: HipEngine.can_split_up, the Python schedule's decision -- the predicate AND AGGMG_DIST_OVERLAP = 1"""
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    n, ratios, ms = shape_of(case)
    nPre, nPost = sweeps
    kinds = D.smoother_kinds(smoother, len(ratios))

    def rank_fn(rank, comm):
        ctx = mg.Context(0)
        layout = D.RankLayout(n, ratios, ms, nranks, rank, nPre, nPost, gs=(smoother == "blockGS"),
                              smoothers=None if smoother in ("blockJac", "blockGS") else kinds)
        engine = nh.build_local_engine(mg, D, r["Ho"], layout, ctx, comm, smoother)
        assert all(engine.H.structured_levels()) and engine.Hc.coarse_info()['on_device']
        if schedule == "native":
            dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        else:
            dv = D.DistributedVCycle(engine, layout, comm)
        b = torch.from_numpy(nh.local_vector(layout, r["b"])).to(engine.dev)
        x = torch.from_numpy(nh.poisoned_ghosts(layout, r["x0"])).to(engine.dev)
        y = engine.new(layout.local_dofs(0))
        outs = []
        for _ in range(NCYC):
            dv.vcycle(x, b, y, nPre, nPost, ALPHA, overlap_next=True)
            x, y = y, x
            torch.cuda.synchronize()
            outs.append(x.cpu().numpy()[layout.owned_slice(0)].copy())
        f = dict(own=layout.own[0], loc=list(layout.loc), chunked=bool(dv.chunked), exchanges=int(dv.exchanges),
                 dictionary=engine.H.dictionary_levels(), can_split=bool(engine.H.can_split_up(nPost)),
                 split_taken=bool(engine.can_split_up(nPost)))
        if facts is not None:
            f.update(facts(engine, layout, dv))
        comm.barrier()
        if hasattr(dv, "free"):
            dv.free()
        return outs, f

    out = _thread_ranks(nranks, rank_fn)
    m0 = ms[0]
    xs = []
    for c in range(NCYC):
        x = np.full(r["N"], np.nan)
        for outs, f in out:
            lo, hi = f["own"]
            x[lo * m0:hi * m0] = outs[c]
        xs.append(x)
    return xs, [f for _, f in out]


def _bits(xs, ss, what):
    """assertion 3"""
    for c, (x, s) in enumerate(zip(xs, ss), 1):
        d = float(np.max(np.abs(x - s)))
        print(f"[dist-nonuniform] {what} cycle {c}: max |partitioned - single GPU| = {d:.3e}")
        assert _same(x, s), (what, c, d)


# ---- block-Jacobi, the library's schedule ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,nranks,sweeps", [("c34_small", 3, (3, 3)), ("c34_small", 3, (1, 2)), ("c34", 8, (3, 3)),
                                                ("p3_1024", 4, (3, 3)), ("p5_1024", 4, (3, 3))],
                         ids=["c34_small-x3-V33", "c34_small-x3-V12", "c34-x8-V33", "p3_1024-x4-V33", "p5_1024-x4-V33"])
def test_native_schedule_block_jacobi(mg, world, case, nranks, sweeps):
    """NativeDistributedVCycle(collectives="torch"), overlap_next on, thread ranks.  c34_small x 3: the smallest shape
    with a two-sided rank, every local level within a dictionary's 1024 records (asserted).  c34 x 8: six two-sided
    ranks, 256 owned fine elements against 160 ghosts.  p3_1024 / p5_1024 x 4: few classes, 256 mod 3 = 256 mod 5 = 1,
    so the ranks start at different phases of the period; the device's class counts are those of
    periodic_helpers.input_classes on every rank's slices (asserted)."""
    r = world.ref(case)
    xr = world.oracle_cycles(case, sweeps)
    xs1 = world.single_cycles(case, "blockJac", sweeps)          # (assertion 1 inside)

    def facts(engine, layout, dv):
        if case not in ph.CASES:
            return {}
        import types
        S = nh.slice_local(r["Ho"], layout)
        Hl = types.SimpleNamespace(mStiffness=S.A, mInterpolation=S.L,
                                   mSmoothers=[types.SimpleNamespace(mBlockInds=i) for i in S.inds])
        return dict(proxy={k: ph.input_classes(Hl, k)[0] for k in range(len(S.inds))})

    xs, fs = _partitioned(mg, r, case, nranks, "blockJac", sweeps, facts=facts)
    for rank, f in enumerate(fs):
        print(f"[dist-nonuniform] {case} x{nranks} rank {rank}: {f}")
        assert not f["chunked"]
        if case == "c34_small":
            assert sorted(f["dictionary"]) == [0, 1, 2], f
        if case in ph.CASES:
            assert f["dictionary"] == f["proxy"] and min(f["proxy"].values()) >= ph.CASES[case][5], f
    _against_the_oracle(r, case, xs, xr, f"partitioned {case} x{nranks} V{sweeps}")
    _bits(xs, xs1, f"{case} x{nranks} V{sweeps}")


@pytest.mark.parametrize("case,nranks,schedule", [("c34", 2, "native")], ids=["c34-x2-native"])
def test_fine_level_over_the_dictionary_cap(mg, world, monkeypatch, case, nranks, schedule):
    """The plain per-element arrays: a local fine level of more than 1024 distinct records takes no dictionary, and
    its launches read operator, inverse and transfer arrays by element offset -- the form in which a rank's offset or a
    tile subset of the split ascent is an index into per-element data.  Every case above is within the cap on every
    rank (c34 x 8 has 256 + 2 x 80 = 416 local records).  c34 x 2: 1024 owned + 80 ghosts = 1104 on both ranks, the
    library's schedule.  Level 0 is absent from dictionary_levels() on every rank and on the single-GPU hierarchy
    (asserted); the three assertions as everywhere.  Both ranks are one-sided: a two-sided rank over the cap needs
    n >= 2880 on three ranks, and at that size the single-GPU cycle itself misses ITERATE_TOL against the oracle
    (2.3e-10 after the first cycle, measured; the coarsest operator of 180 blocks is worse conditioned), so that shape
    would need a reference-against-reference bound of its own and is not run here."""
    monkeypatch.setenv("AGGMG_DIST_OVERLAP", "1" if schedule == "python" else "0")
    r = world.ref(case)
    xr = world.oracle_cycles(case)
    xs1 = world.single_cycles(case)          # (assertion 1 inside)
    assert 0 not in world.single(case).dictionary_levels()
    xs, fs = _partitioned(mg, r, case, nranks, schedule=schedule)
    for rank, f in enumerate(fs):
        print(f"[dist-nonuniform] over the cap {case} x{nranks} {schedule} rank {rank}: {f}")
        assert f["loc"][0][1] - f["loc"][0][0] > nh.DICTIONARY_CAP and 0 not in f["dictionary"], f
        assert sorted(f["dictionary"]) == [1, 2] and f["can_split"] and not f["chunked"], f
        assert f["split_taken"] == (schedule == "python"), f
    assert nranks < 3 or (fs[1]["loc"][0][0] > 0 and fs[1]["loc"][0][1] < shape_of(case)[0])      # a two-sided rank
    _against_the_oracle(r, case, xs, xr, f"partitioned, over the cap {case} x{nranks} {schedule}")
    _bits(xs, xs1, f"over the cap {case} x{nranks} {schedule}")


@pytest.mark.parametrize("coarse_overlap", ["0", "1"])
def test_chunked_coarsest_solve(mg, world, monkeypatch, coarse_overlap):
    """c34 x 4: 128 coarsest blocks of 2 rows, 32 per rank.  AGGMG_CR_TAIL_ROWS = 64 and AGGMG_DIST_COARSE_CHUNK_LOG2 = 2
    make the replicated solver plan chunks of 4 blocks (two levels to eliminate before 32 blocks x 2 rows fit the tail),
    8 per rank: every rank eliminates the chunks of its own block range (aggmg_coarse_chunk_forward / _backward_dev with
    blk_lo > 0), the boundary system of 32 blocks is gathered chunk-interleaved, the coarse ghosts are exchanged -- with
    the exchange in both places (AGGMG_DIST_COARSE_OVERLAP).  Exchanges: cycle 1 x0 + boundary system + coarse ghosts +
    prefetch, cycles 2, 3 three each (as test_distributed_gpu.py::test_four_ranks_overlapped_interface_exchange): 10.
    The single-GPU run (built without these settings) plans its own solve, so bit equality does not apply
    (test_distributed_gpu.py::test_eight_ranks_config4_match_single_gpu says why); the bounds against the oracle hold,
    and the difference to the single-GPU iterate stays within that test's 1e-6 of its scale."""
    case, nranks = "c34", 4
    r = world.ref(case)
    xs1 = world.single_cycles(case)          # (before the settings below: the single-GPU hierarchy plans without them)
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "64")
    monkeypatch.setenv("AGGMG_DIST_COARSE_CHUNK_LOG2", "2")
    monkeypatch.setenv("AGGMG_DIST_COARSE_OVERLAP", coarse_overlap)
    xs, fs = _partitioned(mg, r, case, nranks)
    for rank, f in enumerate(fs):
        print(f"[dist-nonuniform] chunked {case} x{nranks} rank {rank}: {f}")
        assert f["chunked"] and f["exchanges"] == 10, f
    _against_the_oracle(r, case, xs, world.oracle_cycles(case), f"partitioned, chunked {case} x{nranks} overlap {coarse_overlap}")
    for c, (x, s) in enumerate(zip(xs, xs1), 1):
        d = float(np.max(np.abs(x - s)))
        print(f"[dist-nonuniform] chunked cycle {c}: max |partitioned - single GPU| = {d:.3e} of {float(np.max(np.abs(s))):.3e}")
        assert d <= 1e-6 * float(np.max(np.abs(s)))


# ---- the Python schedule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("schedule,overlap,p2p", [("python", "0", "1"), ("python", "1", "1"), ("python", "0", "0"),
                                                  ("python", "1", "0"), ("native", "0", "0")])
def test_python_schedule_and_exchange_forms(mg, world, monkeypatch, schedule, overlap, p2p):
    """DistributedVCycle on the HIP engine, c34_small x 3: AGGMG_DIST_OVERLAP = 1 takes the split ascent
    (aggmg_vcycle_up_split_dev: the tiles at the two ends of the local domain on a second stream, then the middle) and
    the prefetched interface exchange, 0 the plain ascent; AGGMG_DIST_P2P is read by the library's schedule only
    (neighbour messages, or 0: pack, all-gather, unpack), so the last case runs that one with it off."""
    monkeypatch.setenv("AGGMG_DIST_OVERLAP", overlap)
    monkeypatch.setenv("AGGMG_DIST_P2P", p2p)
    case, nranks = "c34_small", 3
    r = world.ref(case)
    xs, fs = _partitioned(mg, r, case, nranks, schedule=schedule)
    what = f"{schedule} schedule {case} x{nranks} overlap {overlap} p2p {p2p}"
    _against_the_oracle(r, case, xs, world.oracle_cycles(case), what)
    _bits(xs, world.single_cycles(case), what)
    assert all(f["can_split"] for f in fs)
    if schedule == "python":      # the split ascent ran exactly where the flag asks for it
        assert all(f["split_taken"] == (overlap == "1") for f in fs), fs


# ---- two gloo processes ----------------------------------------------------------------------------------------------------------
def _gloo_worker(rank, nranks, port, case, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
    import torch
    import torch.distributed as dist
    import aggmg_oracle as o
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=nranks)
    try:
        n, ratios, ms = shape_of(case)
        Ho, b = jh.build(o, case, True)
        x0 = o.splitmix_normal(len(b), jh.X0_SEED)
        ctx = mg.Context(0)
        comm = D.Comm(nranks, rank, staged=True)
        layout = D.RankLayout(n, ratios, ms, nranks, rank)
        engine = nh.build_local_engine(mg, D, Ho, layout, ctx, comm)
        assert all(engine.H.structured_levels()) and engine.Hc.coarse_info()['on_device']
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        bd = torch.from_numpy(nh.local_vector(layout, b)).to(engine.dev)
        x = torch.from_numpy(nh.poisoned_ghosts(layout, x0)).to(engine.dev)
        y = engine.new(layout.local_dofs(0))
        outs = []
        for _ in range(NCYC):
            dv.vcycle(x, bd, y, overlap_next=True)
            x, y = y, x
            torch.cuda.synchronize()
            outs.append(x.cpu().numpy()[layout.owned_slice(0)].copy())
        q.put((rank, layout.own[0], outs, dv.exchanges))
    finally:
        dist.destroy_process_group()


def test_two_gloo_processes(mg, world):
    """the spawn path: two processes, gloo, host-staged collectives, c34_small (this process holds the single-GPU
    hierarchy: three GPU processes alive)"""
    import torch.multiprocessing as mp
    from test_distributed_cpu import free_port
    _guard()
    case = "c34_small"
    r = world.ref(case)
    xr, xs1 = world.oracle_cycles(case), world.single_cycles(case)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(k, 2, port, case, q)) for k in range(2)]
    for pr in procs:
        pr.start()
    # the results are taken BEFORE the joins: a rank's three owned slices are more than the queue's pipe holds, and a
    # process whose queue has not been drained does not exit
    import queue
    got = []
    try:
        for _ in range(2):
            got.append(q.get(timeout=240))
    except queue.Empty:
        pass
    for pr in procs:
        pr.join(60)
    if any(pr.is_alive() for pr in procs):
        for pr in procs:
            pr.kill()
        _fault.append("a gloo rank did not finish within its time limit")
    assert not _fault, _fault
    assert all(pr.exitcode == 0 for pr in procs) and len(got) == 2, ([pr.exitcode for pr in procs], len(got))
    got.sort(key=lambda t: t[0])
    xs = [np.full(r["N"], np.nan) for _ in range(NCYC)]
    for rank, (lo, hi), outs, nex in got:
        # x0 + coarse gather + prefetch, then twice coarse gather + prefetch (the thread ranks' count for this schedule)
        assert nex == 7, (rank, nex)
        for c in range(NCYC):
            xs[c][lo * 4:hi * 4] = outs[c]
    _against_the_oracle(r, case, xs, xr, f"two gloo processes {case}")
    _bits(xs, xs1, f"two gloo processes {case}")


# ---- block Gauss-Seidel ----------------------------------------------------------------------------------------------------------
def test_block_gauss_seidel(mg, world):
    """RankLayout(..., gs=True) on c34 x 8: 256 owned fine elements per rank against a halo of 160 per side; the colours
    are the parity of the LOCAL element index, so every local range starts on an even element (asserted).  The oracle
    side is BlockGaussSeidelRB on the oracle's blocks, as tests/test_gpu_blockgs.py."""
    from agglomerationmultigrid1d_amd import distributed as D
    case, nranks = "c34", 8
    n, ratios, ms = shape_of(case)
    assert D.halo_widths(ratios, 3, 3, gs=True)[0] == 160
    r = world.ref(case)
    xr = world.oracle_cycles(case, gs=True)
    xs1 = world.single_cycles(case, "blockGS")          # (assertion 1 inside)
    xs, fs = _partitioned(mg, r, case, nranks, "blockGS")
    for f in fs:
        assert all(lo % 2 == 0 for lo, _ in f["loc"][:-1]), f
        assert f["own"][1] - f["own"][0] == 256
    _against_the_oracle(r, case, xs, xr, f"partitioned blockGS {case} x{nranks}")
    _bits(xs, xs1, f"blockGS {case} x{nranks}")


# ---- element-patch smoothers -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["patchSchwarz0", "patchGS0"])
def test_element_patch_smoothers(mg, world, smoother):
    """c34 x 4 with the layout sized by smoothers=smoother_kinds(...): against the single-GPU hierarchy of the same
    construction, bit for bit as tests/test_gpu_dist_patch.py::test_partitioned_cycle_is_bitwise_the_single_gpu_cycle
    (the library's predicate, asserted: a multiplicative fine level can take the one-launch split ascent, which the
    library's schedule then does under overlap_next; a hybrid one cannot and takes the plain ascent under the same flag)"""
    case, nranks = "c34", 4
    r = world.ref(case)
    xs1 = world.single_cycles(case, smoother)
    assert all(np.all(np.isfinite(x)) for x in xs1)
    xs, fs = _partitioned(mg, r, case, nranks, smoother)
    for f in fs:
        assert f["can_split"] == smoother.startswith("patchGS") and f["chunked"] == fs[0]["chunked"], f
    _bits(xs, xs1, f"{smoother} {case} x{nranks}")
    # (and the cycle is a multigrid cycle: it reduces the oracle's residual as the block-Jacobi one does)
    res = [float(np.linalg.norm(r["A"] @ x - r["b"])) for x in xs]
    print(f"[dist-nonuniform] {smoother}: ||A x_k - b|| = {res}")
    assert res[2] < res[1] < res[0]


# ---- the outer loops ---------------------------------------------------------------------------------------------------------------
def _solver_rank(mg, r, case, nranks, rank, comm, sweeps=(3, 3)):
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    n, ratios, ms = shape_of(case)
    ctx = mg.Context(0)
    layout = D.RankLayout(n, ratios, ms, nranks, rank, sweeps[0], sweeps[1])
    engine = nh.build_local_engine(mg, D, r["Ho"], layout, ctx, comm)
    dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
    return dv, layout, engine, torch.from_numpy(nh.local_vector(layout, r["b"])).to(engine.dev)


def _gather(r, out, m0=4):
    x = np.full(r["N"], np.nan)
    for res in out:
        (lo, hi), got = res[-2], res[-1]
        x[lo * m0:hi * m0] = got
    return x


def test_partitioned_multigrid_loop(mg, world):
    """distributed.multigrid, check_every = 1, c34_small x 3 against aggmg_multigrid_dev on the whole-range hierarchy, at
    the bounds of test_distributed_gpu.py::test_eight_ranks_partitioned_multigrid_loop_matches_single_gpu: the same cycle
    count, one history on every rank bit for bit, equal to the single-GPU one to rtol 1e-10 / atol 1e-13 ||b||, the
    owned iterate bitwise the single-GPU iterate"""
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    case, nranks, maxiter = "c34_small", 3, 30
    r = world.ref(case)
    Hg = world.single(case)
    ctx2 = Hg.ctx
    bg = ctx2.to_device(np.array(r["b"]))
    nb = float(np.linalg.norm(r["b"]))
    _, _, hist = mg.multigrid_dev(Hg, ctx2.to_device(np.zeros(r["N"])), bg, 6, 1e-30)
    tol = 0.5 * (hist[2] + hist[3]) / nb
    xg, itg, resg = mg.multigrid_dev(Hg, ctx2.to_device(np.zeros(r["N"])), bg, maxiter, tol)
    assert itg == 4, (itg, hist)
    ref = xg.download()

    def rank_fn(rank, comm):
        dv, layout, engine, b = _solver_rank(mg, r, case, nranks, rank, comm)
        x, it, res = D.multigrid(dv, engine.new(layout.local_dofs(0)), b, maxiter, tol, check_every=1)
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)].copy()
        comm.barrier()
        dv.free()
        return it, res, layout.own[0], got

    out = _thread_ranks(nranks, rank_fn)
    print(f"[dist-nonuniform] multigrid: {out[0][0]} cycles (single GPU {itg}), res {out[0][1]} single GPU {list(resg)}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg and res == out[0][1], (rank, it, itg)
        assert np.allclose(res, resg, rtol=1e-10, atol=1e-13 * nb), (rank, res, resg)
    assert _same(_gather(r, out), ref)


def test_partitioned_pcg(mg, world):
    """distributed.pcg on c34_small x 3 against mg.pcg on the whole-range hierarchy, at the bounds of
    test_distributed_pcg_gpu.py::test_partitioned_pcg_matches_single_gpu_pcg: tolerance midway between entries 7 and 8
    of the single-GPU history, the same count, one history on every rank bit for bit, within
    test_distributed_pcg_cpu.HIST_RTOL = 1.61e-11 of the single-GPU one, the gathered iterate's true residual within
    10 gap_g + floor of the last entry (gap_g: the single-GPU run's own gap; floor = 10 eps || |b| + |A| |x| ||)"""
    import torch
    from test_distributed_pcg_cpu import HIST_RTOL
    from agglomerationmultigrid1d_amd import distributed as D
    case, nranks = "c34_small", 3
    r = world.ref(case)
    Hg, A, bg = world.single(case), r["A"], np.array(r["b"])
    nb = float(np.linalg.norm(bg))
    _, _, hist = mg.pcg(Hg, bg, maxiter=12, tol=1e-30)
    tol = 0.5 * (hist[6] + hist[7]) / nb
    xg, itg, resg = mg.pcg(Hg, bg, maxiter=30, tol=tol)
    assert 6 <= itg <= 10, (itg, hist)
    true_g = float(np.linalg.norm(bg - A @ xg))
    gap_g = abs(true_g - resg[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(xg)))

    def rank_fn(rank, comm):
        dv, layout, engine, b = _solver_rank(mg, r, case, nranks, rank, comm)
        x, it, res = D.pcg(dv, b, maxiter=30, tol=tol)
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)].copy()
        comm.barrier()
        dv.free()
        return it, res, layout.own[0], got

    out = _thread_ranks(nranks, rank_fn)
    xp = _gather(r, out)
    true = float(np.linalg.norm(bg - A @ xp))
    res0 = np.array(out[0][1])
    rel = float(np.max(np.abs(res0 - np.array(resg)[:len(res0)]) / np.array(resg)[:len(res0)]))
    print(f"[dist-nonuniform] pcg: iterations {out[0][0]} (single GPU {itg}); history within {rel:.3e} (bound {HIST_RTOL:.2e}); last "
          f"res {res0[-1]:.9e}, true residual {true:.9e}; single GPU gap {gap_g:.3e}, floor {floor:.3e}; "
          f"||x - x_single|| / ||x|| = {float(np.linalg.norm(xp - xg) / np.linalg.norm(xg)):.3e}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg, (rank, it, itg)
        assert res == out[0][1], rank
    assert len(res0) <= 8 and rel <= HIST_RTOL
    assert abs(true - res0[-1]) <= 10 * gap_g + floor


def test_partitioned_fgmres(mg, world):
    """distributed.fgmres with V(2,1), restart 30, on c34_small x 3 against mg.fgmres on the whole-range hierarchy, in
    the form of test_distributed_fgmres_gpu.py::test_partitioned_fgmres_matches_single_gpu_fgmres: the same count, one
    history on every rank bit for bit, the history within ten times the reference-against-reference drift of THIS shape
    (block-Jacobi V(2,1) on this mesh: 4.60e-12 measured in tests/test_distributed_nonuniform_cpu.py, bound 4.6e-11; that
    test's shapes are patch smoothers on the uniform mesh, whose figures do not belong here), the gathered iterate's
    true residual within 10 gap_g + floor of the last entry.  The tolerance is the geometric mean of two consecutive
    entries of the single-GPU history, the last pair within 8 entries that is a factor 1.5 apart (that test's
    stop_tolerance asks for a factor 3, which this cycle does not give on this mesh: the oracle's model history is 427,
    411, 220, 141, 127, 108, 58.2, 56.7 -- entries 6 and 7; the tolerance then sits a factor 1.36 from either, against
    a history bound of 4.6e-11: a movement within the bound cannot change the count)."""
    import torch
    from test_distributed_nonuniform_cpu import FGMRES_V21_HIST_RTOL
    from agglomerationmultigrid1d_amd import distributed as D
    case, nranks, sweeps = "c34_small", 3, (2, 1)
    r = world.ref(case)
    Hg, A, bg = world.single(case), r["A"], np.array(r["b"])
    nb = float(np.linalg.norm(bg))
    kw = dict(restart=30, nPre=2, nPost=1, alpha=ALPHA)
    _, _, hist = mg.fgmres(Hg, bg, maxiter=10, tol=1e-30, **kw)
    counts = [k for k in range(2, 9) if hist[k - 2] >= 1.5 * hist[k - 1]]
    assert counts, hist
    tol = math.sqrt(hist[counts[-1] - 2] * hist[counts[-1] - 1]) / nb
    xg, itg, resg = mg.fgmres(Hg, bg, maxiter=50, tol=tol, **kw)
    assert itg == counts[-1], (itg, hist)
    true_g = float(np.linalg.norm(bg - A @ xg))
    gap_g = abs(true_g - resg[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(xg)))

    def rank_fn(rank, comm):
        dv, layout, engine, b = _solver_rank(mg, r, case, nranks, rank, comm, sweeps)
        x, it, res = D.fgmres(dv, b, maxiter=50, tol=tol, **kw)
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)].copy()
        comm.barrier()
        dv.free()
        return it, res, layout.own[0], got

    out = _thread_ranks(nranks, rank_fn)
    xp = _gather(r, out)
    true = float(np.linalg.norm(bg - A @ xp))
    res0 = np.array(out[0][1])
    rel = float(np.max(np.abs(res0 - np.array(resg)[:len(res0)]) / np.array(resg)[:len(res0)]))
    print(f"[dist-nonuniform] fgmres: iterations {out[0][0]} (single GPU {itg}); history within {rel:.3e} (bound "
          f"{FGMRES_V21_HIST_RTOL:.2e}); last entry {res0[-1]:.9e}, true residual {true:.9e}; single GPU gap {gap_g:.3e}, "
          f"floor {floor:.3e}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg == len(res), (rank, it, itg)
        assert res == out[0][1], rank
    assert len(res0) <= 8 and rel <= FGMRES_V21_HIST_RTOL
    assert abs(true - res0[-1]) <= 10 * gap_g + floor
