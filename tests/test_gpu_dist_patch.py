"""Element-patch smoothers on the element-partitioned cycle, on the GPU: the one-launch split ascent of a multiplicative
patch level against the plain two-launch ascent, bit for bit; the library's partitioned schedule (csrc/dist.hip) with
patch levels on thread ranks (and once on two gloo processes) against the single-GPU cycle, bit for bit; its refusals;
distributed.pcg / distributed.multigrid around the partitioned patchGS cycle against the single-GPU solvers.

Every multi-rank step runs on threads joined under a time limit; after a device failure or a time limit nothing more of
this module starts (`_fault`)."""
import ctypes
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is loaded: the process then holds one HIP runtime, torch's)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
RATIOS, ALPHA = (4, 2, 2), 2.0 / 3.0
VARIANTS = ("patchGS0", "patchGS", "patchSchwarz0", "patchSchwarz")
_fault = []          # why nothing more may start on the GPU from this module


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _guard():
    if _fault:
        pytest.fail(f"not started: an earlier GPU step of this module failed ({_fault[0]})")


def _thread_ranks(world, fn, limit=240):
    """fn(rank, comm) on `world` <= 8 ThreadComm ranks (threads of this process, one library context each)"""
    from agglomerationmultigrid1d_amd import distributed as D
    _guard()
    assert world <= 8
    g = D.ThreadGroup(world)
    out, errs = [None] * world, []

    def one(r):
        try:
            out[r] = fn(r, D.ThreadComm(g, r))
        except BaseException:
            import traceback
            errs.append((r, traceback.format_exc()))
            g.barrier.abort()

    ts = [threading.Thread(target=one, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(limit)
    if any(t.is_alive() for t in ts):
        _fault.append("a rank did not finish within its time limit")
        g.barrier.abort()
    elif errs and ("HIP error" in errs[0][1] or "illegal memory" in errs[0][1]):
        _fault.append("a library call failed on the device")
    assert not _fault, _fault
    assert not errs, errs[0][1]
    return out


def _plan(ctx, m, nsweeps):
    """(tile elements, owned, halo, max sweeps) of the multiplicative sweep launch (C ABI aggmg_patch_gs_tile_plan)"""
    v = [ctypes.c_int(0) for _ in range(4)]
    ctx.check(ctx.lib.aggmg_patch_gs_tile_plan(int(m), int(nsweeps), *[ctypes.byref(x) for x in v]))
    return tuple(x.value for x in v)


# ---- 1. the split ascent --------------------------------------------------------------------------------------------------
def _external_hierarchy(mg, ctx, U, variant):
    from agglomerationmultigrid1d_amd import _lib
    n = U.nlevels
    ops = [mg.DeviceOperator(U.stiffness_csc(k), _lib.OP_STIFFNESS, ctx) for k in range(n)]
    sms = []
    for k in range(n - 1):
        inds = U.descriptor(k).mBlockInds
        if variant.startswith("patchGS") and (k == 0 or not variant.endswith("0")):
            sms.append(mg.ElementPatchGaussSeidel(ops[k], inds.shape[0], inds.shape[1], ctx=ctx))
        elif variant.startswith("patchSchwarz") and (k == 0 or not variant.endswith("0")):
            sms.append(mg.ElementPatchSchwarz(ops[k], inds.shape[0], inds.shape[1], ctx=ctx))
        else:
            sms.append(mg.BlockJacobi(ops[k], inds, ctx))
    Ls = [mg.DeviceOperator(U.interpolation_csc(k), _lib.OP_TRANSFER, ctx) for k in range(n - 1)]
    return mg.MeshHierarchy([U.descriptor(k) for k in range(n)], ops, sms, Ls, ctx=ctx, keep_host=False,
                            coarse_mode=_lib.COARSE_EXTERNAL)


@pytest.mark.parametrize("dictionary", [0, 1])
@pytest.mark.parametrize("variant", ["patchGS0", "patchGS"])
@pytest.mark.parametrize("p,tile", [(3, 192), (1, 512), (2, 340)])
def test_split_ascent_is_bitwise_the_plain_ascent(oracle, mg, p, tile, variant, dictionary):
    """aggmg_vcycle_up_split_dev on a multiplicative patch fine level -- the coarser levels, then ONE launch for the tiles
    at the two ends and one for the middle -- against aggmg_vcycle_up_dev (zero-sweep fused prolongation + sweep launch):
    the parts in both orders on a NaN-filled output, for nPost = 1, 3 and the most one launch takes, head / tail pairs
    at 0, at ne, on and beside tile boundaries, crossed, and a partitioned run's; with and without the operator dictionary;
    alpha and a list of distinct weights."""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    _guard()
    ne, m = 1024, p + 1
    U = UniformDgAggHierarchy(ne, p=p, pAgg=1, ratios=RATIOS)
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, dictionary)
    H = _external_hierarchy(mg, ctx, U, variant)
    assert bool(H.mSmoothers[0].dictionary_classes) == bool(dictionary)
    te, _, _, smax = _plan(ctx, m, 1)
    assert te == tile and smax >= 3
    N = ne * m
    b = ctx.to_device(U.rhs())
    x0 = ctx.to_device(oracle.splitmix_normal(N, 5))
    rp, sp_, nc = H.coarse_buffers()
    sol = oracle.splitmix_normal(nc, 6)

    def descend(nsw):
        H.vcycle_down_dev(x0, b, nsw, ALPHA)
        ctx.check(ctx.lib.aggmg_memcpy_h2d(ctx.handle, sp_, sol.ctypes.data, nc * 8))

    for weights in (None, [0.9, 0.55, 0.7, 0.45, 0.8, 0.6, 0.5, 0.65]):
        for nPost in sorted({1, 3, smax}):
            if weights is not None:
                for k in range(U.nlevels - 1):
                    H.set_sweep_weights(k, weights[:nPost], [w + 0.01 * k for w in weights[:nPost]])
            assert H.can_split_up(nPost)
            owned = _plan(ctx, m, nPost)[1]
            descend(nPost)
            ref = ctx.alloc(N)
            H.vcycle_up_dev(b, ref, nPost, ALPHA)
            ref = ref.download()
            assert np.isfinite(ref).all()
            W0 = 96
            pairs = [(0, ne), (0, 0), (ne, ne), (1, ne - 1), (owned, ne - owned), (owned + 1, ne - owned - 1),
                     (owned - 1, ne - owned + 1), (2 * owned, 3 * owned), (3 * owned + 1, 2 * owned - 1), (700, 100),
                     (W0 + W0, ne - 2 * W0)]
            for head, tail in pairs:
                for order in ((1, 2), (2, 1)):
                    descend(nPost)
                    out = ctx.to_device(np.full(N, np.nan))
                    H.vcycle_up_split_dev(b, out, head, tail, 0, nPost, ALPHA)
                    for part in order:
                        H.vcycle_up_split_dev(b, out, head, tail, part, nPost, ALPHA)
                    assert np.array_equal(out.download(), ref), (weights is not None, nPost, head, tail, order)
    H.free()


@pytest.mark.parametrize("variant,nPost_of_smax", [("patchSchwarz0", 0), ("patchSchwarz", 0), ("patchGS0", 1), ("patchGS0", None)])
def test_no_split_where_the_one_launch_ascent_does_not_apply(oracle, mg, variant, nPost_of_smax):
    """hybrid patch levels, a sweep count that is chunked (max + 1) and nPost = 0 report "no split" from every part and
    launch nothing: the output stays as it was"""
    from agglomerationmultigrid1d_amd._lib import UnsupportedError
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    _guard()
    ne, p = 1024, 3
    U = UniformDgAggHierarchy(ne, p=p, pAgg=1, ratios=RATIOS)
    ctx = mg.Context(0)
    H = _external_hierarchy(mg, ctx, U, variant)
    smax = _plan(ctx, p + 1, 1)[3]
    nPost = 0 if nPost_of_smax is None else (3 if nPost_of_smax == 0 else smax + nPost_of_smax)
    assert not H.can_split_up(nPost)
    N = ne * (p + 1)
    b = ctx.to_device(U.rhs())
    H.vcycle_down_dev(ctx.to_device(oracle.splitmix_normal(N, 5)), b, 3, ALPHA)
    out = ctx.to_device(np.full(N, np.nan))
    for part in (0, 1, 2):
        with pytest.raises(UnsupportedError, match="split ascent"):
            H.vcycle_up_split_dev(b, out, 192, ne - 192, part, nPost, ALPHA)
    assert np.isnan(out.download()).all()
    H.free()


# ---- 2. the partitioned cycle ----------------------------------------------------------------------------------------------
_single = {}


def _single_gpu_cycles(mg, n, p, variant, nPre, nPost, cycles=3):
    """three cycles from zero of the single-GPU hierarchy build_device_hierarchy(U, ctx, smoother=variant): computed once"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    key = (n, p, variant, nPre, nPost, cycles)
    if key not in _single:
        Ug = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=RATIOS)
        ctx2 = mg.Context(0)
        Hg = build_device_hierarchy(Ug, ctx2, smoother=variant)
        bg = ctx2.to_device(Ug.rhs())
        xa, xb = ctx2.to_device(np.zeros(len(Ug.rhs()))), ctx2.alloc(len(Ug.rhs()))
        for _ in range(cycles):
            Hg.vcycle_dev(xa, bg, xb, nPre, nPost, ALPHA)
            xa, xb = xb, xa
        ref = xa.download()
        ref.setflags(write=False)
        Hg.free()
        _single[key] = ref
    return _single[key]


def _partitioned_cycles(mg, world, n, p, variant, nPre, nPost, schedule="native", cycles=3):
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    ref = _single_gpu_cycles(mg, n, p, variant, nPre, nPost, cycles)
    kinds = D.smoother_kinds(variant, len(RATIOS))

    def rank_fn(rank, comm):
        ctx = mg.Context(0)
        layout = D.RankLayout(n, RATIOS, [p + 1, 2, 2, 2], world, rank, nPre, nPost, smoothers=kinds)
        engine, U = D.build_local_uniform(n, p, 1, RATIOS, layout, ctx, comm, smoother=variant)
        assert all(engine.H.structured_levels()) and engine.Hc.coarse_info()['on_device']
        if schedule == "native":
            dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        else:
            dv = D.DistributedVCycle(engine, layout, comm)
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        x, y = engine.new(layout.local_dofs(0)), engine.new(layout.local_dofs(0))
        for _ in range(cycles):
            dv.vcycle(x, b, y, nPre, nPost, ALPHA, overlap_next=True)
            x, y = y, x
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)]
        lo, hi = layout.own[0]
        ref_own = ref[lo * (p + 1):hi * (p + 1)]
        res = (float(np.max(np.abs(got - ref_own))), float(np.max(np.abs(ref_own))), bool(dv.chunked), int(dv.exchanges),
               engine.H.can_split_up(nPost))
        comm.barrier()
        if hasattr(dv, "free"):
            dv.free()
        return res

    return _thread_ranks(world, rank_fn)


@pytest.mark.parametrize("nPre,nPost", [(3, 3), (1, 2)])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("world,n", [(2, 2048), (8, 2**13)])
def test_partitioned_cycle_is_bitwise_the_single_gpu_cycle(mg, world, n, variant, nPre, nPost):
    """the library's schedule (NativeDistributedVCycle, torch collectives) on thread ranks, overlap_next on -- the split
    ascent where the fine level is multiplicative, the plain one under the same flag where it is hybrid: after three
    cycles the owned values are exactly those of the single-GPU cycle of build_device_hierarchy(U, ctx, smoother=...).
    The coarse route (chunked or gathered) is whatever the layout gives, the same on every rank."""
    out = _partitioned_cycles(mg, world, n, 3, variant, nPre, nPost)
    for rank, (err, scale, chunked, nex, split) in enumerate(out):
        assert err == 0.0, (rank, err, scale)
        assert chunked == out[0][2] and split == variant.startswith("patchGS")
        assert nex >= 4      # (the first interface exchange and a coarse gather per cycle at least)


@pytest.mark.parametrize("overlap", ["0", "1"])
@pytest.mark.parametrize("variant", ["patchGS0", "patchSchwarz0"])
def test_python_schedule_with_and_without_the_overlapped_exchange(mg, monkeypatch, variant, overlap):
    """DistributedVCycle on the HIP engine, 2 ranks: AGGMG_DIST_OVERLAP = 1 takes the split ascent and the second stream
    where HipEngine.can_split_up says so (the library's predicate), 0 the plain ascent -- the same bits"""
    monkeypatch.setenv("AGGMG_DIST_OVERLAP", overlap)
    out = _partitioned_cycles(mg, 2, 2048, 3, variant, 3, 3, schedule="python")
    for rank, (err, scale, _, _, _) in enumerate(out):
        assert err == 0.0, (rank, err, scale)


def test_partitioned_cycle_with_chunked_pre_sweeps(mg):
    """nPre = 9: two sweep launches per level at m = 4 (and at m = 2), 2 ranks, n = 2^13"""
    out = _partitioned_cycles(mg, 2, 2**13, 3, "patchGS0", 9, 3)
    for rank, (err, scale, _, _, split) in enumerate(out):
        assert err == 0.0 and split, (rank, err, scale)


def _gloo_worker(rank, world, port, n, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import torch
    import torch.distributed as dist
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        p, variant = 3, "patchGS0"
        ctx = mg.Context(0)
        comm = D.Comm(world, rank, staged=True)
        layout = D.RankLayout(n, RATIOS, [p + 1, 2, 2, 2], world, rank, smoothers=D.smoother_kinds(variant, 3))
        engine, U = D.build_local_uniform(n, p, 1, RATIOS, layout, ctx, comm, smoother=variant)
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        x, y = engine.new(layout.local_dofs(0)), engine.new(layout.local_dofs(0))
        for _ in range(3):
            dv.vcycle(x, b, y, overlap_next=True)
            x, y = y, x
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)]
        ref = _single_gpu_cycles(mg, n, p, variant, 3, 3)
        lo, hi = layout.own[0]
        q.put((rank, float(np.max(np.abs(got - ref[lo * (p + 1):hi * (p + 1)]))), dv.exchanges))
    finally:
        dist.destroy_process_group()


def test_two_gloo_processes_match_single_gpu():
    import torch.multiprocessing as mp
    from test_distributed_cpu import free_port
    _guard()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, 2048, q)) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(300)
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    for rank, err, nex in sorted(q.get() for _ in range(2)):
        assert err == 0.0, (rank, err)


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_reason(mg):
    """through the front end, each an UnsupportedError with the reason in its message: ghost layers sized for V(1,1) and a
    V(3,3) cycle; a patchGS level whose local range starts on an odd element; a patch smoother on the generic route"""
    import torch
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd import distributed as D
    from agglomerationmultigrid1d_amd._lib import UnsupportedError
    p, n = 3, 2048

    def thin(rank, comm):
        ctx = mg.Context(0)
        layout = D.RankLayout(n, RATIOS, [p + 1, 2, 2, 2], 2, rank, 1, 1, smoothers=D.smoother_kinds("patchGS0", 3))
        engine, U = D.build_local_uniform(n, p, 1, RATIOS, layout, ctx, comm, smoother="patchGS0")
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        x, y = engine.new(layout.local_dofs(0)), engine.new(layout.local_dofs(0))
        dv.vcycle(x, b, y, 1, 1, ALPHA)                       # what the layers were sized for
        with pytest.raises(UnsupportedError, match="ghost layers too thin"):
            dv.vcycle(x, b, y, 3, 3, ALPHA)
        comm.barrier()
        dv.free()
        return True

    assert all(_thread_ranks(2, thin))

    # ratios (3,), 105 elements per rank: rank 1 starts on the odd element 105 - W, W even for no smoother list that
    # lacks a two-colour smoother -- a hybrid list gives the odd start that a patchGS level is then refused on
    n3, r3 = 210, (3,)

    def local_hierarchy(layout, ctx, make):
        from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
        U = UniformDgAggHierarchy(n3, p=p, pAgg=1, ratios=r3, elem_range=layout.loc[0])
        ops = [mg.DeviceOperator(U.stiffness_csc(k), _lib.OP_STIFFNESS, ctx) for k in range(2)]
        inds = U.descriptor(0).mBlockInds
        Ls = [mg.DeviceOperator(U.interpolation_csc(0), _lib.OP_TRANSFER, ctx)]
        return mg.MeshHierarchy([U.descriptor(k) for k in range(2)], ops, [make(ops[0], inds.shape[0], inds.shape[1], ctx)], Ls,
                                ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_EXTERNAL)

    def odd_and_generic(rank, comm):
        ctx = mg.Context(0)
        layout = D.RankLayout(n3, r3, [p + 1, 2], 2, rank, 1, 1, smoothers=["patchSchwarz"])
        engine, _ = D.build_local_uniform(n3, p, 1, r3, layout, ctx, comm, smoother="patchSchwarz")
        if rank == 1:
            assert layout.loc[0][0] % 2 == 1
            Hgs = local_hierarchy(layout, ctx, lambda A, m_, ne_, c: mg.ElementPatchGaussSeidel(A, m_, ne_, ctx=c))
            with pytest.raises(UnsupportedError, match="must start on an even element"):
                D.NativeDistributedVCycle(D.HipEngine(Hgs, engine.Hc, ctx), layout, comm, collectives="torch")
        Hw = local_hierarchy(layout, ctx, lambda A, m_, ne_, c: mg.ElementPatchSchwarz(A, m_, ne_, width=3, ctx=c))
        assert not Hw.mSmoothers[0].fused
        with pytest.raises(UnsupportedError, match="generic route"):
            D.NativeDistributedVCycle(D.HipEngine(Hw, engine.Hc, ctx), layout, comm, collectives="torch")
        comm.barrier()
        return True

    assert all(_thread_ranks(2, odd_and_generic))


# ---- 4. the solvers around the partitioned patchGS cycle ----------------------------------------------------------------------
def _solver_rank(mg, n, p, world, rank, comm):
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    ctx = mg.Context(0)
    layout = D.RankLayout(n, RATIOS, [p + 1, 2, 2, 2], world, rank, smoothers=D.smoother_kinds("patchGS", 3))
    engine, U = D.build_local_uniform(n, p, 1, RATIOS, layout, ctx, comm, smoother="patchGS")
    dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
    return dv, layout, engine, torch.from_numpy(np.array(U.rhs())).to(engine.dev)


def test_partitioned_pcg_on_patch_gs_matches_single_gpu_pcg(mg):
    """distributed.pcg around the partitioned patchGS cycle, 8 thread ranks, n = 2^13, against mg.pcg on one GPU with a
    tolerance midway between two consecutive entries of the single-GPU history: the same count on every rank and on one
    GPU, histories identical across ranks, within the bound test_dist_patch_cpu derives (ten times what splitting the
    oracle's own sums moves its history, 2.18e-10), and the gathered iterate's true residual within 10 gap_g + floor of
    the last entry (gap_g: the single-GPU run's own gap between recurrence and true residual; floor = 10 eps || |b| + |A|
    |x| ||, the rounding of forming b - A x on the host)"""
    import torch
    from test_dist_patch_cpu import PCG_HIST_RTOL
    from agglomerationmultigrid1d_amd import distributed as D
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    _guard()
    world, n, p = 8, 2**13, 3
    Ug = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=RATIOS)
    ctx2 = mg.Context(0)
    Hg = build_device_hierarchy(Ug, ctx2, smoother="patchGS")
    A = Ug.stiffness_csc(0).tocsr()
    bg = np.array(Ug.rhs())
    nb = float(np.linalg.norm(bg))
    _, _, hist = mg.pcg(Hg, bg, maxiter=6, tol=1e-30)
    tol = 0.5 * (hist[2] + hist[3]) / nb
    xg, itg, resg = mg.pcg(Hg, bg, maxiter=30, tol=tol)
    Hg.free()
    assert itg == 4, (itg, hist)
    true_g = float(np.linalg.norm(bg - A @ xg))
    gap_g = abs(true_g - resg[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(xg)))

    def rank_fn(rank, comm):
        dv, layout, engine, b = _solver_rank(mg, n, p, world, rank, comm)
        x, it, res = D.pcg(dv, b, maxiter=30, tol=tol)
        torch.cuda.synchronize()
        got = x.cpu().numpy()[layout.owned_slice(0)]
        comm.barrier()
        dv.free()
        return it, res, layout.own[0], got

    out = _thread_ranks(world, rank_fn)
    xp = np.empty(len(bg))
    for it, res, (lo, hi), got in out:
        xp[lo * (p + 1):hi * (p + 1)] = got
    true = float(np.linalg.norm(bg - A @ xp))
    res0 = np.array(out[0][1])
    rel = float(np.max(np.abs(res0 - np.array(resg)[:len(res0)]) / np.array(resg)[:len(res0)]))
    print(f"patchGS pcg: iterations {out[0][0]} (single GPU {itg}); history within {rel:.3e} (bound {PCG_HIST_RTOL:.2e}); last res "
          f"{res0[-1]:.9e}, true residual {true:.9e}; single GPU gap {gap_g:.3e}, floor {floor:.3e}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg, (rank, it, itg)
        assert res == out[0][1], rank
    assert rel <= PCG_HIST_RTOL
    assert abs(true - res0[-1]) <= 10 * gap_g + floor


def test_partitioned_multigrid_on_patch_gs_matches_single_gpu(mg):
    """distributed.multigrid over the partitioned patchGS cycle, 8 thread ranks, n = 2^13, against aggmg_multigrid_dev on
    one GPU: the same cycle count, the same history on every rank (equal to the single-GPU one to the order of its
    sums), the owned iterate exact"""
    import torch
    from agglomerationmultigrid1d_amd import distributed as D
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    _guard()
    world, n, p, maxiter = 8, 2**13, 3, 30
    Ug = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=RATIOS)
    ctx2 = mg.Context(0)
    Hg = build_device_hierarchy(Ug, ctx2, smoother="patchGS")
    N = len(Ug.rhs())
    bg = ctx2.to_device(Ug.rhs())
    _, _, hist = mg.multigrid_dev(Hg, ctx2.to_device(np.zeros(N)), bg, 6, 1e-30)
    tol = 0.5 * (hist[2] + hist[3]) / np.linalg.norm(Ug.rhs())
    xg, itg, resg = mg.multigrid_dev(Hg, ctx2.to_device(np.zeros(N)), bg, maxiter, tol)
    assert itg == 4
    ref = xg.download()
    Hg.free()

    def rank_fn(rank, comm):
        dv, layout, engine, b = _solver_rank(mg, n, p, world, rank, comm)
        x, it, res = D.multigrid(dv, engine.new(layout.local_dofs(0)), b, maxiter, tol)
        torch.cuda.synchronize()
        lo, hi = layout.own[0]
        got, want = x.cpu().numpy()[layout.owned_slice(0)], ref[lo * (p + 1):hi * (p + 1)]
        comm.barrier()
        dv.free()
        return it, res, float(np.max(np.abs(got - want)))

    out = _thread_ranks(world, rank_fn)
    for rank, (it, res, err) in enumerate(out):
        assert it == itg and res == out[0][1], (rank, it, itg)
        assert np.allclose(res, resg, rtol=1e-10, atol=1e-13 * np.linalg.norm(Ug.rhs())), (rank, res, resg)
        assert err == 0.0, (rank, err)
