"""The K-column cycle's level bookkeeping (aggmg_vcycle_multi_dev): which vector a level reads and
writes, with which column stride, on the hierarchies the other K-column suites leave open -- two levels (level 0 prolongs
straight from the coarsest solution, no post-smoothed vector exists anywhere), zero sweep counts on block-tridiagonal
levels, a work space that grows and is shared between hierarchies -- and the argument errors of the K-column entry points,
text for text.

Every comparison is bitwise per column against vcycle_dev on the same hierarchy.  Every K-column call runs on NaN-filled
buffers of leading dimension N + 3 with one column more than K: a read of a padding row poisons the result, a write to one
is seen.  All shapes are tiny (64 fine elements; the chain hierarchies 16)."""
import ctypes
import gc
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 3, 9)
KMAX = max(KS)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


@pytest.fixture(scope="module")
def ctx_all(mg):
    """a context with every opt-in K-column family on"""
    from agglomerationmultigrid1d_amd import _lib
    c = mg.Context(0)
    for o in (_lib.OPT_PATCH_MULTI, _lib.OPT_PATCH_SCHWARZ_MULTI, _lib.OPT_CHAIN_MULTI):
        c.set_option(o, 1)
    return c


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _uniform(ctx, p, ratios, smoother="blockJac", n=64):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    return build_device_hierarchy(UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios), ctx, smoother=smoother)


def _free_all(H):
    sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
    H.free()
    for x in sms + ops + Ls:
        if hasattr(x, "free"):
            x.free()


def _single(H, X0, B, nPre=3, nPost=3):
    """column by column through the single-vector device cycle"""
    c = H.ctx
    N, K = B.shape
    out = np.empty((N, K))
    xo = c.alloc(N)
    for j in range(K):
        x0 = None if X0 is None else c.to_device(X0[:, j])
        H.vcycle_dev(x0, c.to_device(B[:, j]), xo, nPre, nPost)
        out[:, j] = xo.download()
    return out


def _multi(H, X0, B, nPre=3, nPost=3):
    """the K-column device cycle on NaN-filled buffers of leading dimension N + 3 with K + 1 columns"""
    c = H.ctx
    N, K = B.shape
    ld = N + 3

    def up(A):
        pad = np.full((ld, K + 1), np.nan, order="F")
        pad[:N, :K] = A
        return c.to_device(pad.ravel(order="F"))

    dB = up(B)
    dX0 = None if X0 is None else up(X0)
    dX = c.to_device(np.full(ld * (K + 1), np.nan))
    try:
        H.vcycle_multi_dev(dX0, dB, dX, K, ld, nPre, nPost)
        out = dX.download().reshape((ld, K + 1), order="F")
    finally:
        for v in (dB, dX0, dX):
            if v is not None:
                v.free()
    assert np.isnan(out[N:, :]).all(), "rows past N were written"
    assert np.isnan(out[:, K]).all(), "the column past K was written"
    assert np.isfinite(out[:N, :K]).all(), "a padding row or column was read"
    return out[:N, :K]


def _columns(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, KMAX)), rng.standard_normal((N, KMAX))


def _check(H, sweeps, info=None):
    """every K, with and without an initial guess, bit for bit against the single-column cycle of every column;
    info: what multi_info's first entry has to say for a sweep pair (default: in groups)"""
    N = H._ops[0].shape[0]
    B, X0 = _columns(N, N + 11 * H.nlevels)
    for nPre, nPost in sweeps:
        want = True if info is None else info[(nPre, nPost)]
        for guess in (X0, None):
            R = _single(H, guess, B, nPre, nPost)
            for K in KS:
                fused, group = H.multi_info(K, nPre, nPost)
                print(f"levels {H.nlevels} V({nPre},{nPost}) K {K}: multi_info {(fused, group)}")
                assert (fused, group) == ((True, min(K, 8)) if want else (False, 1)), (nPre, nPost, K, fused, group)
                X = _multi(H, None if guess is None else guess[:, :K], B[:, :K], nPre, nPost)
                for j in range(K):
                    assert _same(X[:, j], R[:, j]), (nPre, nPost, K, guess is not None, j, float(np.max(np.abs(X[:, j] - R[:, j]))))


# ---- 1. two levels: level 0 prolongs from the coarsest solution ----------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("smoother", ["blockJac", "patchGS0", "patchSchwarz0"])
def test_two_levels_dg(mg, ctx_all, smoother, p):
    """block-Jacobi, multiplicative patch and hybrid patch level 0 above the coarsest level, ratios = (4,)"""
    H = _uniform(ctx_all, p, (4,), smoother)
    try:
        assert H.nlevels == 2
        _check(H, [(3, 3), (1, 2)])
    finally:
        _free_all(H)


@pytest.mark.parametrize("ps,nDG", [((2, 1), 0), ((1,), 1)])
def test_two_levels_chain(mg, oracle, ctx_all, ps, nDG):
    """one CG chain level above the coarsest: degree 2 over a degree-1 coarsest level (block-ordered vectors longer than
    N), and degree 1 over an agglomerated DG p = 0 coarsest level"""
    Ho, b = oracle.build_cg_hierarchy(16, ps=ps, nDG=nDG, pDG=0 if nDG else None)
    H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx_all)
    try:
        assert H.level_kinds() == ['fused_chain', 'coarsest'], H.level_kinds()
        _check(H, [(3, 3), (1, 2)])
    finally:
        H.free()


# ---- 2. three and four levels of the block-Jacobi family, zero sweep counts -------------------------------------------------
# multi_info's answer on these shapes as recorded from the commit before the driver was restructured: a block-Jacobi level
# runs in column groups at zero sweeps too (its launch is then the transfer alone)
ZERO_SWEEP_INFO = {(0, 3): True, (3, 0): True, (0, 0): True}


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("ratios", [(4, 2), (4, 2, 2)])
def test_zero_sweep_counts(mg, ctx_all, ratios, p):
    H = _uniform(ctx_all, p, ratios)
    try:
        assert H.nlevels == len(ratios) + 1
        _check(H, list(ZERO_SWEEP_INFO), ZERO_SWEEP_INFO)
    finally:
        _free_all(H)


# ---- 3. the work space grows once and is shared -----------------------------------------------------------------------------
def _settle(ctx):
    gc.collect()
    ctx.synchronize()


def _growth(ctx, shapes):
    """K = 2, 11, 3 on the hierarchies of `shapes`, used alternately: every call bitwise; -> (bytes after the K = 11 round,
    bytes after the K = 3 round)"""
    from agglomerationmultigrid1d_amd.api import device_memory
    Hs = [_uniform(ctx, 3, r) for r in shapes]
    try:
        cases = []
        for H in Hs:
            N = H._ops[0].shape[0]
            rng = np.random.default_rng(H.nlevels)
            B, X0 = rng.standard_normal((N, 11)), rng.standard_normal((N, 11))
            cases.append((H, B, X0, _single(H, X0, B)))
        held = []
        for K in (2, 11, 3):
            for H, B, X0, R in cases:
                assert H.multi_info(K)[0]
                X = _multi(H, X0[:, :K], B[:, :K])
                for j in range(K):
                    assert _same(X[:, j], R[:, j]), (H.nlevels, K, j)
            _settle(ctx)
            held.append(device_memory())
        assert held[1][1] > held[0][1], held   # (the K = 11 round grew the vectors of the K = 2 round)
        return held[1], held[2]
    finally:
        for H in Hs:
            _free_all(H)


@pytest.mark.parametrize("shapes", [((4, 2),), ((4,), (4, 2, 2))])
def test_workspace_growth(mg, ctx_all, shapes):
    from agglomerationmultigrid1d_amd.api import device_memory
    _growth(ctx_all, shapes)   # (the context's own work vectors grow on first use and stay)
    _settle(ctx_all)
    start = device_memory()
    grown, after = _growth(ctx_all, shapes)
    assert after == grown, (grown, after)
    assert grown[1] > start[1]
    _settle(ctx_all)
    assert device_memory() == start


# ---- 4. argument errors, text for text --------------------------------------------------------------------------------------
def _raises(mg, c, text, status):
    with pytest.raises(mg.ArgumentError, match=re.escape(text)):
        c.check(status())


def test_error_texts_vcycle_multi(mg, ctx_all):
    c = ctx_all
    H = _uniform(c, 3, (4, 2))
    try:
        N, K = H._ops[0].shape[0], 2
        dB, dX0, dX = (mg.DeviceMatrix(c, N, K) for _ in range(3))
        dB.upload(np.ones((N, K)))

        def call(x0=dX0, b=dB, x=dX, ncols=K, ld=N, nPre=3, nPost=3):
            return lambda: c.lib.aggmg_vcycle_multi_dev(c.handle, H.handle, None if x0 is None else x0.ptr, None if b is None else b.ptr,
                                                        ncols, ld, nPre, nPost, 2.0 / 3.0, x.ptr)

        c.check(call()())   # the call itself is fine
        who = "aggmg_vcycle_multi_dev: "
        _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1))
        _raises(mg, c, who + "ncols must be >= 1", call(ncols=0))
        _raises(mg, c, who + "negative sweep count", call(nPre=-1))
        _raises(mg, c, who + "negative sweep count", call(nPost=-1))
        _raises(mg, c, who + "X must not overlap X0 or B", call(x=dX0))
        _raises(mg, c, who + "X must not overlap X0 or B", call(x=dB))
        _raises(mg, c, who + "NULL argument", call(b=None))
        # the order the checks fire in: NULL, columns, sweep counts, ld, overlap
        _raises(mg, c, who + "NULL argument", call(b=None, ncols=0))
        _raises(mg, c, who + "ncols must be >= 1", call(ncols=0, nPre=-1, ld=N - 1))
        _raises(mg, c, who + "negative sweep count", call(nPre=-1, ld=N - 1))
        _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1, x=dB))
        for x in (dB, dX0, dX):
            x.free()
    finally:
        _free_all(H)


def test_error_texts_coarse_solve_multi(mg, ctx_all):
    c = ctx_all
    H = _uniform(c, 3, (4, 2))
    try:
        N, K = H._ops[-1].shape[0], 2
        dB, dX = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
        dB.upload(np.ones((N, K)))

        def call(b=dB, x=dX, ncols=K, ld=N):
            return lambda: c.lib.aggmg_hier_coarse_solve_multi_dev(c.handle, H.handle, None if b is None else b.ptr, ncols, ld, x.ptr)

        c.check(call()())
        who = "aggmg_hier_coarse_solve_multi_dev: "
        _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1))
        _raises(mg, c, who + "ncols must be >= 1", call(ncols=0))
        _raises(mg, c, who + "X must not overlap B", call(x=dB))
        _raises(mg, c, who + "NULL argument", call(b=None))
        _raises(mg, c, who + "NULL argument", call(b=None, ncols=0))
        _raises(mg, c, who + "ncols must be >= 1", call(ncols=0, ld=N - 1))
        _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1, x=dB))
        for x in (dB, dX):
            x.free()
    finally:
        _free_all(H)


def test_error_texts_smooth_multi(mg):
    import patch_schwarz_model as pm
    c = mg.default_context()
    m, ne, K = 4, 12, 2
    N = m * ne
    op = mg.DeviceOperator(pm.random_block_tridiag(m, ne, "row", 9).tocsc())
    G = mg.ElementPatchGaussSeidel(op, m, ne)
    dB, dU0, dU = (mg.DeviceMatrix(c, N, K) for _ in range(3))
    dB.upload(np.ones((N, K)))
    w = (ctypes.c_double * 1)(2.0 / 3.0)

    def call(u0=dU0, b=dB, u=dU, ncols=K, ld=N, nsweeps=1):
        return lambda: c.lib.aggmg_smooth_multi_dev(c.handle, op.handle, G.handle, None if u0 is None else u0.ptr,
                                                    None if b is None else b.ptr, ncols, ld, w, nsweeps, 0, u.ptr)

    c.check(call()())
    who = "aggmg_smooth_multi_dev: "
    _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1))
    _raises(mg, c, who + "ncols must be >= 1", call(ncols=0))
    _raises(mg, c, who + "negative sweep count or no weights", call(nsweeps=-1))
    _raises(mg, c, who + "U must not overlap U0 or B", call(u=dU0))
    _raises(mg, c, who + "U must not overlap U0 or B", call(u=dB))
    _raises(mg, c, who + "NULL argument", call(b=None))
    _raises(mg, c, who + "NULL argument", call(b=None, ncols=0))
    _raises(mg, c, who + "ncols must be >= 1", call(ncols=0, nsweeps=-1, ld=N - 1))
    _raises(mg, c, who + "negative sweep count or no weights", call(nsweeps=-1, ld=N - 1))
    _raises(mg, c, who + f"ld must be >= N ({N})", call(ld=N - 1, u=dB))
    for x in (G, op, dB, dU0, dU):
        x.free()
