"""distributed.pcg on the GPU: the owned-range kernels alone against NumPy, then conjugate gradients around the
partitioned cycle on thread ranks sharing the GPU against the single-GPU mg.pcg (C ABI aggmg_pcg_dev).

Every GPU step runs on threads that are joined under a time limit of their own; after a fault or a time limit nothing
more of this module starts (`_fault`)."""
import ctypes
import math
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "tests"),) if p not in sys.path]

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
_fault = []          # why nothing more may start on the GPU from this module


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
    elif errs and ("AggmgError" in errs[0][1] or "HIP" in errs[0][1] or "hip" in errs[0][1]):
        _fault.append("a library call failed on the device")
    assert not _fault, _fault
    assert not errs, errs[0][1]
    return out


# ------------------------------------------------------------------------------------------------
# the kernels alone
# ------------------------------------------------------------------------------------------------
N_LOCAL = 700_001
RANGE_SETS = {
    # a long range (more than 1024 slices x 256 threads x 2: the per-thread loop repeats) from an odd offset
    "one": [(1001, 601_002)],
    # a range of length 1 at an odd offset, and one whose length is no multiple of 256
    "two": [(1, 2), (650_000, 650_777)],
    "four": [(1, 2), (3, 260), (1001, 601_002), (650_001, 650_778)],
    "empty_and_whole": [(5, 5), (0, N_LOCAL)],
}


@pytest.fixture(scope="module")
def dev():
    _guard()
    import torch
    import agglomerationmultigrid1d_amd as mg
    ctx = mg.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(5)
    host = {k: rng.standard_normal(N_LOCAL) for k in "xrpqz"}
    for k in "pq":       # 24 significant bits: a * p is exact in double for a 24-bit a, so fma(a, p, x) == x + a * p
        host[k] = host[k].astype(np.float32).astype(np.float64)
    for v in host.values():
        v.setflags(write=False)
    yield ctx, torch, host
    torch.cuda.synchronize()


def _arr(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*[int(v) for v in vals])


def _put(torch, v, offset=0, pad=8):
    """device copy of v as a view `offset` doubles into a buffer with `pad` sentinels on both sides"""
    buf = torch.full((offset + v.size + 2 * pad,), 777.0, dtype=torch.float64, device="cuda")
    view = buf[pad + offset:pad + offset + v.size]
    view.copy_(torch.from_numpy(np.array(v)))
    return buf, view


def _owned_dot(ctx, x, y, ranges):
    out = ctypes.c_double(0.0)
    ctx.check(ctx.lib.aggmg_owned_dot_dev(ctx.handle, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), len(ranges),
                                          _arr([a for a, _ in ranges]), _arr([b for _, b in ranges]), ctypes.byref(out)))
    return out.value


@pytest.mark.parametrize("name", sorted(RANGE_SETS))
@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (1, 0)])
def test_owned_dot_against_fsum(dev, name, offsets):
    """sum over the ranges of x_i y_i against math.fsum of the products: |difference| <= (n + 2) eps sum |x_i y_i| (n terms:
    one rounding per product, at most n - 1 per addition chain whatever the tree).  Vectors 16-byte aligned, both 8 bytes
    off, and one of each (8-byte accesses): the last two walk the same pairs, so they give the same bits.  Twice: the same
    bits from run to run."""
    _guard()
    ctx, torch, host = dev
    ranges = RANGE_SETS[name]
    _, x = _put(torch, host["x"], offsets[0])
    _, y = _put(torch, host["r"], offsets[1])
    torch.cuda.synchronize()
    got = _owned_dot(ctx, x, y, ranges)
    assert got == _owned_dot(ctx, x, y, ranges)
    prods = np.concatenate([host["x"][a:b] * host["r"][a:b] for a, b in ranges])
    want, mag = math.fsum(prods), math.fsum(np.abs(prods))
    print(f"{name} {offsets}: {got!r} vs fsum {want!r}, bound {(prods.size + 2) * EPS * mag:.3e}")
    assert abs(got - want) <= (prods.size + 2) * EPS * mag
    if offsets == (1, 0):
        _, y1 = _put(torch, host["r"], 1)
        torch.cuda.synchronize()
        assert got == _owned_dot(ctx, x, y1, ranges)


def test_owned_dot_argument_checks(dev):
    _guard()
    ctx, torch, host = dev
    import agglomerationmultigrid1d_amd as mg
    _, x = _put(torch, host["x"])
    torch.cuda.synchronize()
    assert _owned_dot(ctx, x, x, []) == 0.0
    with pytest.raises(mg.AggmgError):
        _owned_dot(ctx, x, x, [(0, 1)] * 5)
    with pytest.raises(mg.AggmgError):
        _owned_dot(ctx, x, x, [(3, 2)])
    with pytest.raises(mg.AggmgError):
        _owned_dot(ctx, x, x, [(-1, 2)])
    # two ranges that share a row are refused (by the fused update as well); an empty range overlaps nothing
    with pytest.raises(mg.AggmgError):
        _owned_dot(ctx, x, x, [(10, 20), (19, 30)])
    assert _owned_dot(ctx, x, x, [(10, 20), (15, 15), (20, 30)]) == _owned_dot(ctx, x, x, [(10, 20), (20, 30)])
    _, r = _put(torch, host["r"])
    _, p = _put(torch, host["p"])
    _, q = _put(torch, host["q"])
    torch.cuda.synchronize()
    out = ctypes.c_double(0.0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    for lo, hi in (([0, 5], [6, 9]), ([0], [N_LOCAL + 1])):          # overlapping; past the n rows
        assert ctx.lib.aggmg_pcg_xr_owned_dev(ctx.handle, N_LOCAL, P(x), P(r), P(p), P(q), 0.5, len(lo), _arr(lo), _arr(hi),
                                              ctypes.byref(out)) != 0
    assert np.array_equal(x.cpu().numpy(), host["x"]) and np.array_equal(r.cpu().numpy(), host["r"])


@pytest.mark.parametrize("name", sorted(RANGE_SETS))
@pytest.mark.parametrize("offset", [0, 1])
def test_fused_update_bit_for_bit(dev, name, offset):
    """x += a p, r += a q against NumPy bit for bit: p, q and a carry 24 significant bits, so a * p is exact in double and
    NumPy's x + a * p IS fma(a, p, x).  The sum of the new r_i^2 over the ranges against math.fsum as above.  Nothing is
    written outside the n rows."""
    _guard()
    ctx, torch, host = dev
    ranges = RANGE_SETS[name]
    a = float(np.float32(-0.3712345))
    bx, x = _put(torch, host["x"], offset)
    br, r = _put(torch, host["r"], offset)
    _, p = _put(torch, host["p"], offset)
    _, q = _put(torch, host["q"], offset)
    torch.cuda.synchronize()
    out = ctypes.c_double(0.0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx.check(ctx.lib.aggmg_pcg_xr_owned_dev(ctx.handle, N_LOCAL, P(x), P(r), P(p), P(q), a, len(ranges),
                                             _arr([lo for lo, _ in ranges]), _arr([hi for _, hi in ranges]), ctypes.byref(out)))
    xw = host["x"] + a * host["p"]
    rw = host["r"] + a * host["q"]
    assert np.array_equal(x.cpu().numpy(), xw) and np.array_equal(r.cpu().numpy(), rw)
    for buf in (bx, br):
        h = buf.cpu().numpy()
        assert np.all(h[:8 + offset] == 777.0) and np.all(h[8 + offset + N_LOCAL:] == 777.0)
    sq = np.concatenate([rw[lo:hi] * rw[lo:hi] for lo, hi in ranges])
    want = math.fsum(sq)
    assert abs(out.value - want) <= (sq.size + 2) * EPS * want


def test_fused_update_general_data_within_one_ulp(dev):
    """operands with full mantissas: NumPy rounds a * p before it adds, the kernel's fma does not -- within 1 ulp"""
    _guard()
    ctx, torch, host = dev
    a = 0.1234567890123
    _, x = _put(torch, host["x"])
    _, r = _put(torch, host["r"])
    _, p = _put(torch, host["z"])
    _, q = _put(torch, host["x"], 1)          # (mixed alignment: the 8-byte path)
    torch.cuda.synchronize()
    out = ctypes.c_double(0.0)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    ctx.check(ctx.lib.aggmg_pcg_xr_owned_dev(ctx.handle, N_LOCAL, P(x), P(r), P(p), P(q), a, 1, _arr([0]), _arr([N_LOCAL]),
                                             ctypes.byref(out)))
    for got, base, d in ((x, host["x"], host["z"]), (r, host["r"], host["x"])):
        want = base + a * d
        # 1 ulp of the result, plus the rounding of a * d that NumPy made and the fma did not
        g = got.cpu().numpy()
        assert np.all(np.abs(g - want) <= np.spacing(np.maximum(np.abs(want), np.abs(g))) + 0.5 * np.spacing(np.abs(a * d)))


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (0, 1)])
def test_direction_update_bit_for_bit(dev, offsets):
    """p = z + beta p against NumPy bit for bit (24-bit p and beta: the product is exact)"""
    _guard()
    ctx, torch, host = dev
    beta = float(np.float32(0.8124))
    bp, p = _put(torch, host["p"], offsets[0])
    _, z = _put(torch, host["z"], offsets[1])
    torch.cuda.synchronize()
    ctx.check(ctx.lib.aggmg_pcg_p_dev(ctx.handle, N_LOCAL, ctypes.c_void_p(p.data_ptr()), ctypes.c_void_p(z.data_ptr()), beta))
    ctx.synchronize()
    assert np.array_equal(p.cpu().numpy(), host["z"] + beta * host["p"])
    h = bp.cpu().numpy()
    assert np.all(h[:8 + offsets[0]] == 777.0) and np.all(h[8 + offsets[0] + N_LOCAL:] == 777.0)


# ------------------------------------------------------------------------------------------------
# the loop on thread ranks against the single-GPU pcg
# ------------------------------------------------------------------------------------------------
CASES = {
    "config4_8ranks": dict(config=4, world=8, n=2**16, driver="native"),
    "config5_8ranks": dict(config=5, world=8, n=2**14, driver="native"),
    "config4_2ranks_torch_collectives": dict(config=4, world=2, n=2048, driver="native"),
    "config4_2ranks_python_schedule": dict(config=4, world=2, n=2048, driver="python"),
}
P_DG, RATIOS, PS = 3, (4, 2, 2), (4, 2, 1)


def _single_gpu(case):
    """the global hierarchy, mg.pcg's run on one GPU with a tolerance met after 8 iterations (taken from its own history)"""
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd.uniform import (UniformCgDgHierarchy, UniformDgAggHierarchy, build_device_cg_hierarchy,
                                                      build_device_hierarchy)
    ctx2 = mg.Context(0)
    if case["config"] == 4:
        Ug = UniformDgAggHierarchy(case["n"], p=P_DG, pAgg=1, ratios=RATIOS)
        Hg = build_device_hierarchy(Ug, ctx2)
        A = Ug.stiffness_csc(0).tocsr()
    else:
        Ug = UniformCgDgHierarchy(case["n"], ps=PS)
        Hg = build_device_cg_hierarchy(Ug, ctx2)
        A = Ug.A[0].tocsr()
    bg = np.array(Ug.rhs())
    nb = float(np.linalg.norm(bg))
    _, _, hist = mg.pcg(Hg, bg, maxiter=12, tol=1e-30)
    tol = 0.5 * (hist[6] + hist[7]) / nb
    xg, itg, resg = mg.pcg(Hg, bg, maxiter=30, tol=tol)
    Hg.free()
    return dict(A=A, bg=bg, nb=nb, tol=tol, xg=xg, itg=itg, resg=resg)


def _make_rank(case, rank, comm):
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    ctx = mg.Context(0)
    world, n = case["world"], case["n"]
    if case["config"] == 4:
        layout = D.RankLayout(n, RATIOS, [P_DG + 1, 2, 2, 2], world, rank)
        engine, U = D.build_local_uniform(n, P_DG, 1, RATIOS, layout, ctx, comm)
        glob = np.arange(layout.own[0][0] * (P_DG + 1), layout.own[0][1] * (P_DG + 1))
        loc = np.arange(layout.owned_slice(0).start, layout.owned_slice(0).stop)
    else:
        layout = D.CgRankLayout(n, PS, world, rank, 3, 3)
        engine, U = D.build_local_cg(n, PS, layout, ctx, comm)
        glob, loc = layout.global_index(0), layout.owned_index(0)
        assert len(layout.owned_ranges(0)) == 2
    if case["driver"] == "native":
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
    else:
        dv = D.DistributedVCycle(engine, layout, comm)
    b = torch.from_numpy(np.array(U.rhs())).to(engine.dev)
    return dv, layout, engine, b, glob, loc


@pytest.mark.parametrize("name", sorted(CASES))
def test_partitioned_pcg_matches_single_gpu_pcg(name):
    """distributed.pcg on thread ranks sharing the GPU against mg.pcg on one GPU, tolerance met after 8 iterations (taken
    from the single-GPU history): the same count on every rank and on one GPU; histories identical across ranks bit for
    bit; the history within the tolerance test_distributed_pcg_cpu derives for the shape -- ten times what splitting the
    oracle's own sums into rank-sized pieces moves its history: 1.61e-11 on config 4's shape, 7.24e-7 on config 5's at
    n = 2^14, whose 8 iterations reduce ||r|| by twelve orders and whose entries move accordingly (7.24e-8 reference
    against reference at this very size; 4.2e-8 measured here against the single-GPU run); the gathered owned iterate's
    true residual ||b - A x|| (host, scipy) agrees with the last `res` entry.

    Margin of the last check: ten times the gap the single-GPU run itself shows between its recurrence residual and its
    true residual (gap_g, measured by this test on every run and printed), plus the rounding of forming b - A x in double
    on the host, floor = 10 eps || |b| + |A| |x| ||_2 (rows of at most 10 terms).  What the figures are, and how much the
    check says on each shape:
      config 4, n = 2048:  last res 2.67, gap 7.0e-12 (2.6e-12 of res), floor 1.2e-8: the bound is the floor, and it holds
                           the true residual to 4.6e-9 of res;
      config 4, n = 2^16:  last res 85.6, gap 9.3e-11 (1.1e-12 of res), floor 2.0e-6: 2.4e-8 of res;
      config 5, n = 2^14:  last res 4.305e-10, true residual 7.49e-9 on one GPU (7.53e-9 partitioned): gap 7.1e-9, SIXTEEN
                           times res, floor 2.2e-7.  The recurrence has run below what b - A x can be formed to in double
                           (||b|| = 1.2e3), so on this shape the check is weak: it says only that the true residual of
                           the gathered iterate is below about 3e-7 = 2.4e-10 ||b||, not that it equals res.  What ties
                           this case to the single-GPU run is the history check above.
    The config-4 figures are oracle.pcg_ldiv's on the CPU at these shapes with this test's tolerance rule (the single-GPU
    run of the same recurrence prints its own beside them); the config-5 figures are the single-GPU run's."""
    from test_distributed_pcg_cpu import HIST_RTOL, hist_rtol_config5
    from agglomerationmultigrid1d_amd import distributed as D
    _guard()
    case = CASES[name]
    hist_rtol = HIST_RTOL if case["config"] == 4 else hist_rtol_config5(case["n"])
    ref = _single_gpu(case)
    A, bg, tol, itg, resg = ref["A"], ref["bg"], ref["tol"], ref["itg"], ref["resg"]
    assert 6 <= itg <= 10, itg
    true_g = float(np.linalg.norm(bg - A @ ref["xg"]))
    gap_g = abs(true_g - resg[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(ref["xg"])))

    def rank_fn(rank, comm):
        import torch
        dv, layout, engine, b, glob, loc = _make_rank(case, rank, comm)
        x, it, res = D.pcg(dv, b, maxiter=30, tol=tol)
        torch.cuda.synchronize()
        got = x.cpu().numpy()[loc]
        comm.barrier()
        if hasattr(dv, "free"):
            dv.free()
        return it, res, glob, got

    out = _thread_ranks(case["world"], rank_fn)
    xg = np.empty(len(bg))
    for it, res, glob, got in out:
        xg[glob] = got
    true = float(np.linalg.norm(bg - A @ xg))
    rel = float(np.max(np.abs(np.array(out[0][1]) - np.array(resg)[:len(out[0][1])]) / np.array(resg)[:len(out[0][1])]))
    print(f"{name}: iterations {out[0][0]} (single GPU {itg}); history within {rel:.3e} of the single-GPU one (bound "
          f"{hist_rtol:.2e}); last res {out[0][1][-1]:.9e}, true residual {true:.9e}, gap {abs(true - out[0][1][-1]):.3e}; "
          f"single GPU: last res {resg[-1]:.9e}, true {true_g:.9e}, gap {gap_g:.3e} ({gap_g / resg[-1]:.3e} relative); "
          f"rounding floor {floor:.3e}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg, (rank, it, itg)
        assert res == out[0][1], rank
    assert len(out[0][1]) <= 8 and rel <= hist_rtol
    assert abs(true - out[0][1][-1]) <= 10 * gap_g + floor


def test_argument_handling_and_nonzero_start():
    """nPre != nPost raises; sweep counts above the halo widths raise; maxiter = 0 returns the start vector, 0 and [];
    a nonzero x0 (ghosts wrong on purpose) converges to the same solution: its gathered true residual meets the recurrence's
    last entry with the margin of the test above (gap of the zero-start single-GPU run, times ten, plus the host rounding
    floor)."""
    from agglomerationmultigrid1d_amd import distributed as D
    _guard()
    case = CASES["config4_2ranks_torch_collectives"]
    ref = _single_gpu(case)
    A, bg, nb = ref["A"], ref["bg"], ref["nb"]
    tol = 1e-9
    x0g = np.random.default_rng(3).standard_normal(len(bg))

    def rank_fn(rank, comm):
        import torch
        dv, layout, engine, b, glob, loc = _make_rank(case, rank, comm)
        with pytest.raises(ValueError):
            D.pcg(dv, b, nPre=3, nPost=2)
        with pytest.raises(ValueError):
            D.pcg(dv, b, nPre=4, nPost=4)
        sl = layout.owned_slice(0)
        lo = layout.loc[0][0] * (P_DG + 1)
        x0 = torch.from_numpy(x0g[lo:lo + layout.local_dofs(0)].copy()).to(engine.dev)
        x0[:sl.start] = 5.0
        x0[sl.stop:] = -7.0
        keep = x0.clone()
        torch.cuda.synchronize()
        xs, its, ress = D.pcg(dv, b, x0=x0, maxiter=0)
        assert its == 0 and ress == [] and torch.equal(xs, keep)
        xz, itz, resz = D.pcg(dv, b, maxiter=0)
        assert itz == 0 and resz == [] and not xz.any()
        x, it, res = D.pcg(dv, b, x0=x0, maxiter=60, tol=tol)
        torch.cuda.synchronize()
        assert torch.equal(x0, keep)
        got = x.cpu().numpy()[loc]
        comm.barrier()
        dv.free()
        return it, res, glob, got

    out = _thread_ranks(case["world"], rank_fn)
    xg = np.empty(len(bg))
    for it, res, glob, got in out:
        assert it == len(res) < 60 and res == out[0][1] and res[-1] < tol * nb
        xg[glob] = got
    true = float(np.linalg.norm(bg - A @ xg))
    gap_g = abs(float(np.linalg.norm(bg - A @ ref["xg"])) - ref["resg"][-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(xg)))
    print(f"nonzero x0: {out[0][0]} iterations, last res {out[0][1][-1]:.9e}, true residual {true:.9e}, bound "
          f"{10 * gap_g + floor:.3e}")
    assert abs(true - out[0][1][-1]) <= 10 * gap_g + floor
