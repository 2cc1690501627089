"""distributed.fgmres on the GPU: the fused owned-range passes of its orthogonalisation alone (aggmg_owned_multi_dot_dev,
aggmg_owned_multi_axpy_norm_dev, aggmg_div_scalar_dev) against aggmg_owned_dot_dev and NumPy, then flexible GMRES around
the partitioned cycle on thread ranks sharing the GPU against the single-GPU mg.fgmres (C ABI aggmg_fgmres_dev).

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
    elif errs and any(k in errs[0][1] for k in ("AggmgError", "HIP error", "hipError")):
        _fault.append("a library call failed on the device")
    assert not _fault, (_fault, errs[0][1] if errs else None)
    assert not errs, errs[0][1]
    return out


# ------------------------------------------------------------------------------------------------
# the kernels alone
# ------------------------------------------------------------------------------------------------
N_LOCAL = 700_001
RANGE_SETS = {       # test_distributed_pcg_gpu.py's
    # a long range (more than 1024 slices x 256 threads x 2: the per-thread loop repeats) from an odd offset
    "one": [(1001, 601_002)],
    # a range of length 1 at an odd offset, and one whose length is no multiple of 256
    "two": [(1, 2), (650_000, 650_777)],
    "four": [(1, 2), (3, 260), (1001, 601_002), (650_001, 650_778)],
    "empty_and_whole": [(5, 5), (0, N_LOCAL)],
}
NVECS = [1, 8, 9, 17]                 # one group, a full group, a group and one, two groups and one
LD_EVEN, LD_ODD = N_LOCAL + 3, N_LOCAL + 2
PAD = 8
# (offset of w, offset of V from a 16-byte boundary, ld): 16-byte accesses on even and odd pair grids, then the 8-byte
# path by an odd ld, by a basis off w's alignment, and by both
PLACEMENTS = [(0, 0, LD_EVEN), (1, 1, LD_EVEN), (0, 0, LD_ODD), (1, 0, LD_EVEN), (1, 0, LD_ODD)]


@pytest.fixture(scope="module")
def dev():
    _guard()
    import torch
    import agglomerationmultigrid1d_amd as mg
    ctx = mg.Context(0)
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(7)
    # 24 significant bits in the basis and the coefficients: c * v is exact in double, so fma(c, v, x) == x + c * v
    host = dict(V=rng.standard_normal((max(NVECS), N_LOCAL)).astype(np.float32).astype(np.float64),
                w=rng.standard_normal(N_LOCAL),
                coef=rng.standard_normal(max(NVECS)).astype(np.float32).astype(np.float64))
    for v in host.values():
        v.setflags(write=False)
    yield ctx, torch, host
    torch.cuda.synchronize()


def _arr(vals):
    return (ctypes.c_int64 * max(len(vals), 1))(*[int(v) for v in vals])


def _P(t):
    return ctypes.c_void_p(t.data_ptr())


def _put(torch, v, offset=0):
    """device copy of v as a view `offset` doubles into a buffer with PAD sentinels on both sides"""
    buf = torch.full((offset + v.size + 2 * PAD,), 777.0, dtype=torch.float64, device="cuda")
    view = buf[PAD + offset:PAD + offset + v.size]
    view.copy_(torch.from_numpy(np.array(v)))
    return buf, view


def _put_basis(torch, Vh, nvec, offset, ld):
    """the first nvec rows of Vh at stride ld, `offset` doubles into a sentinel-filled buffer -> (buffer, host image of
    the buffer, tensor whose data_ptr is vector 0)"""
    img = np.full(offset + nvec * ld + 2 * PAD, 777.0)
    for i in range(nvec):
        img[PAD + offset + i * ld:PAD + offset + i * ld + N_LOCAL] = Vh[i]
    buf = torch.from_numpy(img).to("cuda")
    return buf, img, buf[PAD + offset:]


def _sentinels_intact(buf, offset, n=N_LOCAL):
    h = buf.cpu().numpy()
    return bool(np.all(h[:PAD + offset] == 777.0) and np.all(h[PAD + offset + n:] == 777.0))


def _owned_dot(ctx, x, y, ranges):
    out = ctypes.c_double(0.0)
    ctx.check(ctx.lib.aggmg_owned_dot_dev(ctx.handle, _P(x), _P(y), len(ranges), _arr([a for a, _ in ranges]),
                                          _arr([b for _, b in ranges]), ctypes.byref(out)))
    return out.value


def _multi_dot(ctx, V, nvec, ld, w, ranges, check=True):
    out = np.full(nvec, np.nan)
    st = ctx.lib.aggmg_owned_multi_dot_dev(ctx.handle, _P(V) if V is not None else None, nvec, ld,
                                           _P(w) if w is not None else None, len(ranges), _arr([a for a, _ in ranges]),
                                           _arr([b for _, b in ranges]), out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    if check:
        ctx.check(st)
        return out
    return st


def _multi_axpy(ctx, n, V, nvec, ld, coef, w, ranges, want=True, check=True):
    out = ctypes.c_double(np.nan)
    cf = np.ascontiguousarray(coef, dtype=np.float64)
    st = ctx.lib.aggmg_owned_multi_axpy_norm_dev(ctx.handle, n, _P(V), nvec, ld, cf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                 _P(w), len(ranges), _arr([a for a, _ in ranges]), _arr([b for _, b in ranges]),
                                                 ctypes.byref(out) if want else None)
    if check:
        ctx.check(st)
        return out.value
    return st


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("name", sorted(RANGE_SETS))
def test_multi_dot_is_owned_dot_entry_by_entry(dev, name, nvec):
    """entry i == aggmg_owned_dot_dev(w, V_i) on the same ranges, bit for bit, in every placement (16-byte accesses on
    both pair grids; the 8-byte path by an odd ld, by a basis off w's alignment, by both); the same bits twice; the same
    bits in all placements of one pair grid (the 8-byte path walks the 16-byte path's pairs); nothing is written to the
    vectors."""
    _guard()
    ctx, torch, host = dev
    ranges = RANGE_SETS[name]
    by_grid = {}
    for w_off, v_off, ld in PLACEMENTS:
        bw, w = _put(torch, host["w"], w_off)
        bv, img, V = _put_basis(torch, host["V"], nvec, v_off, ld)
        torch.cuda.synchronize()
        got = _multi_dot(ctx, V, nvec, ld, w, ranges)
        assert got.tobytes() == _multi_dot(ctx, V, nvec, ld, w, ranges).tobytes()
        for i in range(nvec):
            assert got[i] == _owned_dot(ctx, w, V[i * ld:], ranges), (w_off, v_off, ld, i)
        assert np.array_equal(bv.cpu().numpy(), img) and _sentinels_intact(bw, w_off)
        assert np.array_equal(w.cpu().numpy(), host["w"])
        by_grid.setdefault(w_off, got)
        assert got.tobytes() == by_grid[w_off].tobytes(), (w_off, v_off, ld)
    prods = np.concatenate([host["V"][0][a:b] * host["w"][a:b] for a, b in ranges])
    want, mag = math.fsum(prods), math.fsum(np.abs(prods))
    for got in by_grid.values():       # (and it is the dot product: owned_dot's bound against math.fsum)
        assert abs(got[0] - want) <= (prods.size + 2) * EPS * mag


@pytest.mark.parametrize("nvec", NVECS)
@pytest.mark.parametrize("name", sorted(RANGE_SETS))
def test_multi_axpy_norm_bit_for_bit(dev, name, nvec):
    """the stored w == the NumPy chain w + c_0 V_0 + ... (ascending) bit for bit: coefficients and basis values carry 24
    significant bits, so every product is exact and NumPy's x + c * v IS fma(c, v, x).  The owned sum of squares within
    (n + 2) eps of math.fsum (n terms: one rounding per square, at most n - 1 per addition chain whatever the tree), the
    same bits twice and in all placements of one pair grid.  Without the sum the stored values are the same.  Nothing
    is written outside the n rows, nothing to the basis."""
    _guard()
    ctx, torch, host = dev
    ranges = RANGE_SETS[name]
    coef = host["coef"][:nvec]
    want = host["w"].copy()
    for i in range(nvec):
        want = want + coef[i] * host["V"][i]
    sq = np.concatenate([want[a:b] * want[a:b] for a, b in ranges])
    ss_want = math.fsum(sq)
    by_grid = {}
    for w_off, v_off, ld in PLACEMENTS:
        bv, img, V = _put_basis(torch, host["V"], nvec, v_off, ld)
        sums = []
        for want_sum in (True, True, False):
            bw, w = _put(torch, host["w"], w_off)
            torch.cuda.synchronize()
            ss = _multi_axpy(ctx, N_LOCAL, V, nvec, ld, coef, w, ranges, want=want_sum)
            ctx.synchronize()
            assert np.array_equal(w.cpu().numpy(), want), (w_off, v_off, ld, want_sum)
            assert _sentinels_intact(bw, w_off)
            if want_sum:
                sums.append(ss)
        assert np.array_equal(bv.cpu().numpy(), img)
        assert sums[0] == sums[1]
        assert abs(sums[0] - ss_want) <= (sq.size + 2) * EPS * ss_want
        by_grid.setdefault(w_off, sums[0])
        assert sums[0] == by_grid[w_off], (w_off, v_off, ld)


def test_multi_axpy_general_data_within_the_chain_bound(dev):
    """operands with full mantissas, 17 vectors: NumPy rounds every product before it adds, the kernel's fma does not --
    per entry within nvec roundings of the chain's largest partial sum (1 ulp of it each, 2 for the two orders)"""
    _guard()
    ctx, torch, host = dev
    nvec, ld = 17, LD_EVEN
    rng = np.random.default_rng(9)
    Vh, coef = rng.standard_normal((nvec, N_LOCAL)), rng.standard_normal(nvec)
    _, _, V = _put_basis(torch, Vh, nvec, 0, ld)
    _, w = _put(torch, host["w"])
    torch.cuda.synchronize()
    _multi_axpy(ctx, N_LOCAL, V, nvec, ld, coef, w, [(0, N_LOCAL)])
    want, big = host["w"].copy(), np.abs(host["w"])
    for i in range(nvec):
        want = want + coef[i] * Vh[i]
        big = np.maximum(big, np.maximum(np.abs(want), np.abs(coef[i] * Vh[i])))
    assert np.all(np.abs(w.cpu().numpy() - want) <= 2 * nvec * EPS * big)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (0, 1), (1, 0)])
def test_div_scalar_bit_for_bit(dev, offsets):
    """v = w / s against NumPy bit for bit (a division: s = 3 has no exact reciprocal), v apart from w at equal and at
    different alignments, and v == w in place; nothing is written outside the n rows"""
    _guard()
    ctx, torch, host = dev
    s = 3.0 * float(np.linalg.norm(host["w"][:1000]))
    assert not np.array_equal(host["w"] / s, host["w"] * (1.0 / s))        # (the reciprocal would show)
    bw, w = _put(torch, host["w"], offsets[0])
    bv, v = _put(torch, np.zeros(N_LOCAL), offsets[1])
    torch.cuda.synchronize()
    ctx.check(ctx.lib.aggmg_div_scalar_dev(ctx.handle, N_LOCAL, _P(w), s, _P(v)))
    ctx.synchronize()
    assert np.array_equal(v.cpu().numpy(), host["w"] / s) and np.array_equal(w.cpu().numpy(), host["w"])
    assert _sentinels_intact(bv, offsets[1]) and _sentinels_intact(bw, offsets[0])
    ctx.check(ctx.lib.aggmg_div_scalar_dev(ctx.handle, N_LOCAL, _P(w), s, _P(w)))
    ctx.synchronize()
    assert np.array_equal(w.cpu().numpy(), host["w"] / s) and _sentinels_intact(bw, offsets[0])


def test_argument_errors_leave_the_vectors_untouched(dev):
    _guard()
    ctx, torch, host = dev
    import agglomerationmultigrid1d_amd as mg
    nvec, ld = 3, LD_EVEN
    bv, img, V = _put_basis(torch, host["V"], nvec, 0, ld)
    bw, w = _put(torch, host["w"])
    torch.cuda.synchronize()
    whole, coef = [(0, N_LOCAL)], host["coef"][:nvec]
    bad_ranges = ([(0, 1)] * 5, [(3, 2)], [(-1, 2)], [(10, 20), (19, 30)])
    # the dots: nvec outside 1 .. 65, ld short of the last range, bad ranges, w inside the basis, NULL
    for kw in (dict(nvec=0), dict(nvec=66), dict(ld=N_LOCAL - 1), dict(w=V[ld:]), dict(V=None), dict(w=None),
               *[dict(ranges=r) for r in bad_ranges]):
        a = dict(V=V, nvec=nvec, ld=ld, w=w, ranges=whole)
        a.update(kw)
        assert _multi_dot(ctx, a["V"], a["nvec"], a["ld"], a["w"], a["ranges"], check=False) == mg._lib.ERR_ARGUMENT, kw
    with pytest.raises(mg.AggmgError):
        _multi_dot(ctx, V, 66, ld, w, whole)
    assert np.array_equal(_multi_dot(ctx, V, nvec, ld, w, []), np.zeros(nvec))        # no range: zeros, no launch
    # the update: the same, ld < n, a range past the n rows, w inside the basis
    for kw in (dict(nvec=0), dict(nvec=66), dict(ld=N_LOCAL - 1), dict(n=-1), dict(w=V[ld + 5:]), dict(ranges=[(0, N_LOCAL + 1)]),
               *[dict(ranges=r) for r in bad_ranges]):
        a = dict(n=N_LOCAL, V=V, nvec=nvec, ld=ld, w=w, ranges=whole)
        a.update(kw)
        assert _multi_axpy(ctx, a["n"], a["V"], a["nvec"], a["ld"], coef, a["w"], a["ranges"], check=False) == mg._lib.ERR_ARGUMENT, kw
    null = ctypes.c_void_p(None)
    out = ctypes.c_double(0.0)
    assert ctx.lib.aggmg_owned_multi_axpy_norm_dev(ctx.handle, N_LOCAL, _P(V), nvec, ld, None, _P(w), 1, _arr([0]), _arr([N_LOCAL]),
                                                   ctypes.byref(out)) == mg._lib.ERR_ARGUMENT
    assert ctx.lib.aggmg_owned_multi_axpy_norm_dev(ctx.handle, N_LOCAL, null, nvec, ld, coef.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                                   _P(w), 1, _arr([0]), _arr([N_LOCAL]), ctypes.byref(out)) == mg._lib.ERR_ARGUMENT
    # the division: NULL, n < 0, a divisor that is 0 or not finite, v overlapping w partly
    for n, src, s, dst in ((N_LOCAL, w, 0.0, V), (N_LOCAL, w, -0.0, V), (N_LOCAL, w, float("inf"), V), (N_LOCAL, w, float("nan"), V),
                           (-1, w, 2.0, V), (N_LOCAL, w, 2.0, None), (N_LOCAL, None, 2.0, V), (N_LOCAL - 8, w, 2.0, w[4:])):
        assert ctx.lib.aggmg_div_scalar_dev(ctx.handle, n, _P(src) if src is not None else None, s,
                                            _P(dst) if dst is not None else None) == mg._lib.ERR_ARGUMENT, (n, s)
    ctx.synchronize()
    assert np.array_equal(bv.cpu().numpy(), img)
    assert np.array_equal(w.cpu().numpy(), host["w"]) and _sentinels_intact(bw, 0)


# ------------------------------------------------------------------------------------------------
# the loop on thread ranks against the single-GPU fgmres
# ------------------------------------------------------------------------------------------------
P_DG, RATIOS, PS, ALPHA = 3, (4, 2, 2), (4, 2, 1), 2.0 / 3.0
# shape: the entry of test_distributed_fgmres_cpu.SHAPES whose sweeps, restart length, entries and history bound apply
CASES = {
    "schwarz0_v33_8ranks": dict(shape="schwarz0_v33", world=8, n=2**13, driver="native"),
    "schwarz0_v33_restart3_8ranks": dict(shape="schwarz0_v33_r3", world=8, n=2**13, driver="native"),
    "schwarz_v21_2ranks_native": dict(shape="schwarz_v21", world=2, n=2048, driver="native"),
    "schwarz_v21_2ranks_python_schedule": dict(shape="schwarz_v21", world=2, n=2048, driver="python"),
    "config5_v21_8ranks": dict(shape="config5_v21", world=8, n=2**14, driver="native"),
}


def _single_gpu(case, s, tol=None):
    """the global hierarchy and mg.fgmres's run on one GPU: the tolerance is met after s['entries'] iterations (taken
    from its own history), or the run is cut there when the restart length is shorter"""
    import agglomerationmultigrid1d_amd as mg
    from test_distributed_fgmres_cpu import stop_tolerance
    from agglomerationmultigrid1d_amd.uniform import (UniformCgDgHierarchy, UniformDgAggHierarchy, build_device_cg_hierarchy,
                                                      build_device_hierarchy)
    ctx2 = mg.Context(0)
    if s["smoother"] is None:
        Ug = UniformCgDgHierarchy(case["n"], ps=PS)
        Hg = build_device_cg_hierarchy(Ug, ctx2)
        A = Ug.A[0].tocsr()
    else:
        Ug = UniformDgAggHierarchy(case["n"], p=P_DG, pAgg=1, ratios=RATIOS)
        Hg = build_device_hierarchy(Ug, ctx2, smoother=s["smoother"])
        A = Ug.stiffness_csc(0).tocsr()
    bg = np.array(Ug.rhs())
    nb = float(np.linalg.norm(bg))
    kw = dict(restart=s["restart"], nPre=s["nPre"], nPost=s["nPost"], alpha=ALPHA)
    if tol is None:
        if s["restart"] < s["entries"]:
            tol, maxiter = 1e-30, s["entries"]
        else:
            _, _, hist = mg.fgmres(Hg, bg, maxiter=s["entries"] + 2, tol=1e-30, **kw)
            tol, maxiter = stop_tolerance(hist, s["entries"], nb), 50
    else:
        maxiter = 60
    kw.update(tol=tol, maxiter=maxiter)
    xg, itg, resg = mg.fgmres(Hg, bg, **kw)
    Hg.free()
    return dict(A=A, bg=bg, nb=nb, kw=kw, xg=xg, itg=itg, resg=resg)


def _make_rank(case, s, rank, comm):
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    ctx = mg.Context(0)
    world, n = case["world"], case["n"]
    if s["smoother"] is None:
        layout = D.CgRankLayout(n, PS, world, rank, s["nPre"], s["nPost"])
        engine, U = D.build_local_cg(n, PS, layout, ctx, comm)
        glob, loc = layout.global_index(0), layout.owned_index(0)
        assert len(layout.owned_ranges(0)) == 2
    else:
        layout = D.RankLayout(n, RATIOS, [P_DG + 1, 2, 2, 2], world, rank, s["nPre"], s["nPost"],
                              smoothers=D.smoother_kinds(s["smoother"], len(RATIOS)))
        engine, U = D.build_local_uniform(n, P_DG, 1, RATIOS, layout, ctx, comm, smoother=s["smoother"])
        glob = np.arange(layout.own[0][0] * (P_DG + 1), layout.own[0][1] * (P_DG + 1))
        loc = np.arange(layout.owned_slice(0).start, layout.owned_slice(0).stop)
    if case["driver"] == "native":
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
    else:
        dv = D.DistributedVCycle(engine, layout, comm)
    b = torch.from_numpy(np.array(U.rhs())).to(engine.dev)
    return dv, layout, engine, b, glob, loc


@pytest.mark.parametrize("name", sorted(CASES))
def test_partitioned_fgmres_matches_single_gpu_fgmres(name):
    """distributed.fgmres on thread ranks sharing the GPU against mg.fgmres on one GPU, the tolerance the geometric mean
    of two consecutive entries of the single-GPU history at least a factor 3 apart (restart 3: cut at 8 entries instead):
    the same count on every rank and on one GPU; histories identical across ranks bit for bit; the history within the
    bound test_distributed_fgmres_cpu derives for the shape -- ten times what summing the model's own dots in 1 .. 8
    rank-sized pieces moves its history; the gathered owned iterate's true residual ||b - A x|| (host, scipy) within
    10 gap_g + floor of the last entry, gap_g the gap the single-GPU run itself shows between its last entry and its true
    residual, floor = 10 eps || |b| + |A| |x| ||_2 the rounding of forming b - A x in double on the host -- exactly
    test_partitioned_pcg_matches_single_gpu_pcg's margin.  The cycles here are the ones distributed.pcg has no answer
    for: hybrid patch levels, and V(2,1)."""
    from test_distributed_fgmres_cpu import SHAPES, hist_rtol
    from agglomerationmultigrid1d_amd import distributed as D
    _guard()
    case = CASES[name]
    s = SHAPES[case["shape"]]
    ref = _single_gpu(case, s)
    A, bg, kw, itg, resg = ref["A"], ref["bg"], ref["kw"], ref["itg"], ref["resg"]
    assert itg == s["entries"], (itg, resg)
    true_g = float(np.linalg.norm(bg - A @ ref["xg"]))
    gap_g = abs(true_g - resg[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(bg) + abs(A) @ np.abs(ref["xg"])))

    def rank_fn(rank, comm):
        import torch
        dv, layout, engine, b, glob, loc = _make_rank(case, s, rank, comm)
        x, it, res = D.fgmres(dv, b, **kw)
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
    res0 = np.array(out[0][1])
    rel = float(np.max(np.abs(res0 - np.array(resg)[:len(res0)]) / np.array(resg)[:len(res0)]))
    print(f"{name}: iterations {out[0][0]} (single GPU {itg}); history within {rel:.3e} of the single-GPU one (bound "
          f"{hist_rtol(case['shape']):.2e}); last entry {res0[-1]:.9e}, true residual {true:.9e}, gap {abs(true - res0[-1]):.3e}; "
          f"single GPU: last entry {resg[-1]:.9e}, true {true_g:.9e}, gap {gap_g:.3e}; rounding floor {floor:.3e}")
    for rank, (it, res, _, _) in enumerate(out):
        assert it == itg == len(res), (rank, it, itg)
        assert res == out[0][1], rank
    assert len(res0) <= 8 and rel <= hist_rtol(case["shape"])
    assert abs(true - res0[-1]) <= 10 * gap_g + floor


def test_argument_handling_and_nonzero_start():
    """restart outside 1 .. 64 and sweep counts above the halo widths raise; maxiter = 0 returns the start vector (zeros
    without one), 0 and []; a nonzero x0 (ghosts wrong on purpose) is left alone and converges to the same solution: its
    gathered true residual meets the last entry with the margin of the test above (gap of the zero-start single-GPU run
    to the same tolerance, times ten, plus the host rounding floor)."""
    from test_distributed_fgmres_cpu import SHAPES
    from agglomerationmultigrid1d_amd import distributed as D
    _guard()
    case = CASES["schwarz_v21_2ranks_native"]
    s = SHAPES[case["shape"]]
    tol = 1e-9
    ref = _single_gpu(case, s, tol=tol)
    A, bg, nb, kw = ref["A"], ref["bg"], ref["nb"], ref["kw"]
    x0g = np.random.default_rng(3).standard_normal(len(bg))

    def rank_fn(rank, comm):
        import torch
        dv, layout, engine, b, glob, loc = _make_rank(case, s, rank, comm)
        for bad in (0, 65):
            with pytest.raises(ValueError):
                D.fgmres(dv, b, restart=bad)
        with pytest.raises(ValueError):
            D.fgmres(dv, b, nPre=3, nPost=1)
        sl = layout.owned_slice(0)
        lo = layout.loc[0][0] * (P_DG + 1)
        x0 = torch.from_numpy(x0g[lo:lo + layout.local_dofs(0)].copy()).to(engine.dev)
        x0[:sl.start] = 5.0
        x0[sl.stop:] = -7.0
        keep = x0.clone()
        torch.cuda.synchronize()
        xs, its, ress = D.fgmres(dv, b, x0=x0, maxiter=0, nPre=s["nPre"], nPost=s["nPost"])
        assert its == 0 and ress == [] and torch.equal(xs, keep)
        xz, itz, resz = D.fgmres(dv, b, maxiter=0, nPre=s["nPre"], nPost=s["nPost"])
        assert itz == 0 and resz == [] and not xz.any()
        x, it, res = D.fgmres(dv, b, x0=x0, **kw)
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
    print(f"nonzero x0: {out[0][0]} iterations, last entry {out[0][1][-1]:.9e}, true residual {true:.9e}, bound "
          f"{10 * gap_g + floor:.3e}")
    assert abs(true - out[0][1][-1]) <= 10 * gap_g + floor
