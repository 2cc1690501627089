"""Flexible GMRES on K right-hand sides in lockstep (aggmg_fgmres_multi_dev, api.fgmres_multi; EXTENSION)
and the K-column passes of its orthogonalisation (aggmg_multi_dot_cols_dev, aggmg_multi_axpy_norm_cols_dev).

Every assertion is a bit-for-bit equality against the single-vector entry points run in the same process: the passes
against Context.multi_dot / Context.multi_axpy_norm on each column alone (which tests/test_gpu_fgmres.py holds equal to
dot / norm2), the solver against fgmres on each column.  No tolerance is chosen anywhere."""
import ctypes
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [1, 255, 256, 257, 4099, 1_000_003]
NVECS = (1, 8, 9, 17)
NCOLS = (1, 3, 8, 9)
POISON = 1e300


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- 1. the passes ---------------------------------------------------------------------------------------------------
class _Bases:
    """max(NVECS) x max(NCOLS) basis vectors of n rows on the device, basis index outer, column inner, with padded
    strides: every column has `pad` rows behind it and every basis index one column more than is used, all POISON.  The
    smaller shapes of a test are the leading basis indices and columns of the same buffers.  (The largest case, 17 x 9
    vectors of 1 000 003 rows, is 1.2 GB on the device; it fitted, so nvec = 17 is not dropped there.)"""

    def __init__(self, ctx, n, seed):
        self.ctx, self.n = ctx, n
        self.nvec, self.ncols = max(NVECS), max(NCOLS)
        self.cstride = n + 5
        self.bstride = (self.ncols + 1) * self.cstride
        self.ldw = n + 3
        rng = np.random.default_rng(seed)
        self.V = np.full((self.nvec, self.ncols + 1, self.cstride), POISON)
        self.V[:, :self.ncols, :n] = rng.random((self.nvec, self.ncols, n)) - 0.5
        self.W = np.full((self.ncols + 1, self.ldw), POISON)
        self.W[:self.ncols, :n] = rng.random((self.ncols, n)) - 0.5
        self.coef = rng.random((self.ncols, self.nvec)) - 0.5
        self.dV = ctx.to_device(self.V.ravel())
        self.dW0 = ctx.to_device(self.W.ravel())       # pristine
        self.dW = ctx.to_device(self.W.ravel())

    def vcol(self, c):
        return self.dV.ptr.value + 8 * c * self.cstride

    def wcol(self, c):
        return self.dW.ptr.value + 8 * c * self.ldw

    def reset_w(self):
        from agglomerationmultigrid1d_amd import api
        api._copy_dev(self.ctx, self.dW.ptr.value, self.dW0.ptr.value, self.W.size)

    def w(self):
        return self.dW.download().reshape(self.W.shape)


@pytest.mark.parametrize("n", NS)
def test_multi_dot_cols_is_multi_dot_per_column(mg, n):
    ctx = mg.default_context()
    S = _Bases(ctx, n, 11)
    ref = np.stack([ctx.multi_dot(S.vcol(c), S.wcol(c), n=n, nvec=S.nvec, ld=S.bstride) for c in range(S.ncols)])
    exact = np.einsum("icr,cr->ci", S.V[:, :S.ncols, :n], S.W[:S.ncols, :n])
    assert np.allclose(ref, exact, rtol=0, atol=1e-12 * max(1, n))           # (the reference itself is what it should be)
    for nvec in NVECS:
        for ncols in NCOLS:
            got = ctx.multi_dot_cols(S.dV, S.dW, n, nvec, ncols, bstride=S.bstride, cstride=S.cstride, ldw=S.ldw)
            assert got.shape == (ncols, nvec)
            assert _same(got, ref[:ncols, :nvec]), (n, nvec, ncols, np.argwhere(got != ref[:ncols, :nvec])[:5])
    again = ctx.multi_dot_cols(S.dV, S.dW, n, S.nvec, S.ncols, bstride=S.bstride, cstride=S.cstride, ldw=S.ldw)
    assert _same(again, ref)                                                  # run to run
    assert _same(S.w(), S.W) and _same(S.dV.download(), S.V.ravel())          # both only read


@pytest.mark.parametrize("n", NS)
def test_multi_axpy_norm_cols_is_multi_axpy_norm_per_column(mg, n):
    ctx = mg.default_context()
    S = _Bases(ctx, n, 12)
    for nvec in NVECS:
        S.reset_w()
        rnorm = np.array([ctx.multi_axpy_norm(S.vcol(c), S.coef[c, :nvec], S.wcol(c), n=n, nvec=nvec, ld=S.bstride)
                          for c in range(S.ncols)])
        rW = S.w()
        assert not _same(rW[:S.ncols, :n], S.W[:S.ncols, :n])
        for ncols in NCOLS:
            S.reset_w()
            norms = ctx.multi_axpy_norm_cols(S.dV, S.coef[:ncols, :nvec], S.dW, n, nvec, ncols, bstride=S.bstride,
                                             cstride=S.cstride, ldw=S.ldw)
            got = S.w()
            assert norms.shape == (ncols,) and _same(norms, rnorm[:ncols]), (n, nvec, ncols)
            assert _same(got[:ncols, :n], rW[:ncols, :n]), (n, nvec, ncols)
            assert _same(got[ncols:], S.W[ncols:]) and _same(got[:, n:], S.W[:, n:])      # other columns, padding rows
            if ncols == 3:      # without the norms: the same columns
                S.reset_w()
                assert ctx.multi_axpy_norm_cols(S.dV, S.coef[:ncols, :nvec], S.dW, n, nvec, ncols, bstride=S.bstride,
                                                cstride=S.cstride, ldw=S.ldw, norm=False) is None
                assert _same(S.w(), got)
    assert _same(S.dV.download(), S.V.ravel())                                # the bases and their padding: only read


def test_cols_pass_arguments(mg):
    ctx = mg.default_context()
    n, nvec, ncols = 8, 3, 2
    dV = ctx.to_device(np.ones(nvec * ncols * n))
    dW = ctx.to_device(np.ones(ncols * n))
    ok = dict(bstride=ncols * n, cstride=n, ldw=n)
    assert _same(ctx.multi_dot_cols(dV, dW, n, nvec, ncols, **ok), np.full((ncols, nvec), 8.0))
    for bad in (dict(nvec=0), dict(nvec=66), dict(ncols=0), dict(bstride=n - 1), dict(cstride=n - 1), dict(ldw=n - 1),
                dict(n=-1)):
        a = dict(n=n, nvec=nvec, ncols=ncols, **ok)
        a.update(bad)
        with pytest.raises(mg.ArgumentError):
            ctx.multi_dot_cols(dV, dW, a["n"], a["nvec"], a["ncols"], bstride=a["bstride"], cstride=a["cstride"], ldw=a["ldw"])
        with pytest.raises(mg.ArgumentError):
            ctx.multi_axpy_norm_cols(dV, np.ones((max(a["ncols"], 1), max(a["nvec"], 1))), dW, a["n"], a["nvec"], a["ncols"],
                                     bstride=a["bstride"], cstride=a["cstride"], ldw=a["ldw"])
    for V, W in ((None, dW), (dV, None)):
        with pytest.raises(mg.ArgumentError):
            ctx.multi_dot_cols(V, W, n, nvec, ncols, **ok)
    with pytest.raises(mg.ArgumentError, match="overlap"):                    # W inside V
        ctx.multi_axpy_norm_cols(dV, np.ones((ncols, nvec)), dV.ptr.value + 8 * n, n, nvec, ncols, **ok)
    assert _same(dV.download(), np.ones(nvec * ncols * n)) and _same(dW.download(), np.ones(ncols * n))
    assert _same(ctx.multi_dot_cols(dV, dW, 0, nvec, ncols, **ok), np.zeros((ncols, nvec)))   # no rows: empty sums


# ---- 2. the solver, on the fused cycle -------------------------------------------------------------------------------
_CASES = {}
TOL = 1e-7
CYCLE = dict(nPre=2, nPost=1)
RUNS = {"restart8": dict(restart=8, maxiter=200), "restart30": dict(restart=30, maxiter=200),
        "restart30_maxiter4": dict(restart=30, maxiter=4)}


def _hier(o, mg, name):
    """-> (Ho, H): oracle hierarchy and its device mirror, built once per module and never modified"""
    if name in _CASES:
        return _CASES[name]
    if name.startswith("dg"):
        Ho, _ = o.build_dg_agg_hierarchy(int(name[2:]), p=3, pAgg=1, nAgg=3, first=4)
    else:                                       # CG p = 4, 2, 1 with hybrid Schwarz, then DG p = 0
        Ho, _ = o.build_cg_hierarchy(int(name[7:]), ps=(4, 2, 1), nDG=1, pDG=0)
        for k in range(3):
            Ho.mSmoothers[k] = o.cg_smoother(Ho.mMeshes[k], Ho.mStiffness[k], "hybridSchwarz")
    _CASES[name] = (Ho, mg.MeshHierarchy.from_reference(Ho))
    return _CASES[name]


def _columns(o, mg):
    """(B, X0), N x 9, built so that the single calls end at different iterations (seeds picked with tests/fgmres_model.py
    on the CPU: the plain columns take 39 .. 56 iterations at this tolerance, the warm-started ones 0, 3 and about 30).
    The first three columns alone already hold a zero count, two distinct positive ones and a finish inside a restart
    cycle, so K = 3 crosses the compaction path as K = 9 does.  Built once and never modified."""
    if "columns" in _CASES:
        return _CASES["columns"]
    Ho, H = _hier(o, mg, "dg48")
    N = Ho.mStiffness[0].shape[0]
    B = np.zeros((N, 9), order="F")
    X0 = np.zeros((N, 9), order="F")
    B[:, 0] = o.splitmix_normal(N, 1)
    # column 1: all zero
    B[:, 2] = o.splitmix_normal(N, 2)                 # nearly there: the single call's solution at 2e-7 -> 3 iterations
    X0[:, 2] = mg.fgmres(H, B[:, 2], restart=30, maxiter=200, tol=2e-7, **CYCLE)[0]
    B[:, 3] = 1e3 * o.splitmix_normal(N, 3)
    B[:, 4] = o.splitmix_normal(N, 4)                 # solved at 1e-8, asked for 1e-7: zero iterations, untouched
    X0[:, 4] = mg.fgmres(H, B[:, 4], restart=30, maxiter=200, tol=1e-8, **CYCLE)[0]
    B[:, 5] = o.splitmix_normal(N, 5)                 # the single call's iterate after 10 iterations: fewer remain
    X0[:, 5] = mg.fgmres(H, B[:, 5], restart=30, maxiter=10, tol=TOL, **CYCLE)[0]
    B[:, 6] = o.splitmix_normal(N, 6)
    X0[:, 6] = o.splitmix_normal(N, 106)
    B[:, 7] = o.splitmix_normal(N, 7)
    B[:, 8] = 1e-3 * o.splitmix_normal(N, 1)
    X0[:, 8] = o.splitmix_normal(N, 108)
    B.setflags(write=False)
    X0.setflags(write=False)
    _CASES["columns"] = (B, X0)
    return B, X0


def _singles(mg, H, B, X0, key, **kw):
    """fgmres on every column, once per (key): [(x, iters, res)]"""
    if key not in _CASES:
        _CASES[key] = [mg.fgmres(H, B[:, j].copy(), x0=None if X0 is None else X0[:, j].copy(), **kw)
                       for j in range(B.shape[1])]
    return _CASES[key]


def _assert_columns_equal(got, ref):
    X, its, res = got
    assert X.shape[1] == len(its) == len(res) == len(ref)
    for j, (xs, its_s, res_s) in enumerate(ref):
        assert its[j] == its_s, (j, list(its), [r[1] for r in ref])
        assert res[j] == res_s, j
        assert _same(X[:, j], xs), j


@pytest.mark.parametrize("run", list(RUNS))
def test_single_calls_end_at_different_iterations(oracle, mg, run):
    """what keeps the compaction path from being skipped silently: on the single-call results the counts include 0, two
    distinct positive values, and a finish that is neither at a restart boundary nor at maxiter -- for the nine columns
    and for the first three"""
    Ho, H = _hier(oracle, mg, "dg48")
    B, X0 = _columns(oracle, mg)
    kw = dict(tol=TOL, **RUNS[run], **CYCLE)
    counts = [r[1] for r in _singles(mg, H, B, X0, run, **kw)]
    print(run, counts)
    for K in (3, 9):
        c = counts[:K]
        assert 0 in c
        assert len({v for v in c if v > 0}) >= 2
        assert any(v > 0 and v % kw["restart"] != 0 and v < kw["maxiter"] for v in c)
    assert counts[1] == 0 and counts[4] == 0
    if run == "restart8":
        assert max(counts) > 3 * 8           # several restarts


@pytest.mark.parametrize("K", [1, 3, 9])
@pytest.mark.parametrize("run", list(RUNS))
def test_fgmres_multi_is_fgmres_per_column(oracle, mg, run, K):
    Ho, H = _hier(oracle, mg, "dg48")
    B9, X9 = _columns(oracle, mg)
    kw = dict(tol=TOL, **RUNS[run], **CYCLE)
    ref = _singles(mg, H, B9, X9, run, **kw)[:K]
    B, X0 = np.array(B9[:, :K], order="F"), np.array(X9[:, :K], order="F")
    got = mg.fgmres_multi(H, B, X0=X0, **kw)
    _assert_columns_equal(got, ref)
    assert _same(B, B9[:, :K]) and _same(X0, X9[:, :K])
    if K > 1:
        assert _same(got[0][:, 1], X9[:, 1]) and got[1][1] == 0          # the zero column: untouched
    if K > 4:
        assert _same(got[0][:, 4], X9[:, 4]) and got[1][4] == 0          # within the tolerance at entry: untouched
    # row-major host arrays: the same call
    _assert_columns_equal(mg.fgmres_multi(H, np.ascontiguousarray(B), X0=np.ascontiguousarray(X0), **kw), ref)
    # DeviceMatrix in, DeviceMatrix out, inputs untouched; work_cols = the cycles the columns needed
    ctx = H.ctx
    dB, dX0 = mg.DeviceMatrix(ctx, B.shape[0], K), mg.DeviceMatrix(ctx, B.shape[0], K)
    dB.upload(B)
    dX0.upload(X0)
    Xd, itd, resd = mg.fgmres_multi(H, dB, X0=dX0, **kw)
    assert isinstance(Xd, mg.DeviceMatrix)
    _assert_columns_equal((Xd.download(), itd, resd), ref)
    assert _same(dB.download(), B) and _same(dX0.download(), X0)
    dX = mg.DeviceMatrix(ctx, B.shape[0], K)
    dX.upload(X0)
    its, res, work = H.fgmres_multi_dev(dB, dX, tol=TOL, **RUNS[run], **CYCLE)
    _assert_columns_equal((dX.download(), its, res), ref)
    assert work == sum(r[1] for r in ref) == int(np.sum(its))


def test_zero_guesses_by_default(oracle, mg):
    Ho, H = _hier(oracle, mg, "dg48")
    B9, _ = _columns(oracle, mg)
    kw = dict(restart=8, maxiter=20, tol=TOL, **CYCLE)
    B = np.array(B9[:, [0, 1, 3]], order="F")
    ref = _singles(mg, H, B, None, "zero guesses", **kw)
    _assert_columns_equal(mg.fgmres_multi(H, B, **kw), ref)
    dB = mg.DeviceMatrix(H.ctx, B.shape[0], 3)
    dB.upload(B)
    Xd, itd, resd = mg.fgmres_multi(H, dB, **kw)
    _assert_columns_equal((Xd.download(), itd, resd), ref)


# ---- 3. hierarchies the K-column cycle and residual do not cover -----------------------------------------------------
def test_fallback_hierarchy_column_by_column(oracle, mg):
    """CG p = 4, 2, 1 with hybrid Schwarz levels: the cycle and the residual run column by column, the same contract"""
    Ho, H = _hier(oracle, mg, "schwarz32")
    N = Ho.mStiffness[0].shape[0]
    B = np.zeros((N, 3), order="F")
    B[:, 0] = oracle.splitmix_normal(N, 1)
    B[:, 2] = 1e3 * oracle.splitmix_normal(N, 2)
    X0 = np.zeros((N, 3), order="F")
    X0[:, 2] = oracle.splitmix_normal(N, 102)
    kw = dict(restart=10, maxiter=200, tol=1e-10, nPre=3, nPost=3)
    ref = _singles(mg, H, B, X0, "schwarz32 singles", **kw)
    counts = [r[1] for r in ref]
    print("schwarz32", counts)
    assert counts[1] == 0 and counts[0] > 0 and counts[2] > 0
    _assert_columns_equal(mg.fgmres_multi(H, B, X0=X0, **kw), ref)


# ---- 4. multiplicative patch levels, option off and on ---------------------------------------------------------------
@pytest.mark.parametrize("on", [0, 1])
def test_patch_levels(oracle, mg, on):
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    ctx = mg.Context(0)
    try:
        ctx.set_option(_lib.OPT_PATCH_MULTI, on)
        U = UniformDgAggHierarchy(64, p=3, pAgg=1, ratios=(4, 2, 2))
        H = build_device_hierarchy(U, ctx, smoother="patchGS0")
        N = H._ops[0].shape[0]
        B = np.zeros((N, 4), order="F")
        B[:, 0] = U.rhs()
        B[:, 1] = oracle.splitmix_normal(N, 1)
        B[:, 3] = 1e3 * oracle.splitmix_normal(N, 2)          # (column 2: zero)
        X0 = np.zeros((N, 4), order="F")
        X0[:, 3] = oracle.splitmix_normal(N, 103)
        kw = dict(restart=5, maxiter=40, tol=1e-9, nPre=2, nPost=1)
        ref = [mg.fgmres(H, B[:, j].copy(), x0=X0[:, j].copy(), **kw) for j in range(4)]
        counts = [r[1] for r in ref]
        print("patchGS0", on, counts)
        assert counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 0
        before = ctx.patch_multi_launches()
        _assert_columns_equal(mg.fgmres_multi(H, B, X0=X0, **kw), ref)
        grown = ctx.patch_multi_launches() - before
        assert (grown > 0) if on else (grown == 0)
    finally:
        ctx.close()


# ---- 5. edges --------------------------------------------------------------------------------------------------------
def _call(c, H, B, X, K, ld, restart=8, maxiter=6, tol=TOL, nPre=2, nPost=1, hist=True, its=True):
    """the C entry itself, so that every argument can be wrong"""
    h = np.zeros(max(1, K) * max(1, maxiter))
    n = np.zeros(max(1, K), dtype=np.int32)
    work = ctypes.c_int64(0)
    c.check(c.lib.aggmg_fgmres_multi_dev(c.handle, H.handle if H is not None else None, ctypes.c_void_p(B), ctypes.c_void_p(X),
                                         K, ld, restart, maxiter, tol, nPre, nPost, 2.0 / 3.0,
                                         h.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if hist else None,
                                         n.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if its else None, ctypes.byref(work)))
    return n, h, work.value


def test_fgmres_multi_edges(oracle, mg):
    from agglomerationmultigrid1d_amd import _lib
    Ho, H = _hier(oracle, mg, "dg48")
    ctx = H.ctx
    B9, X9 = _columns(oracle, mg)
    N = B9.shape[0]
    B, X0 = np.array(B9[:, :3], order="F"), np.array(X9[:, 6:9], order="F")
    # maxiter = 0: nothing happens
    X, its, res = mg.fgmres_multi(H, B, X0=X0, maxiter=0, **CYCLE)
    assert list(its) == [0, 0, 0] and res == [[], [], []] and _same(X, X0)
    # a padded leading dimension, one column more than is used, everything else poisoned
    K, ld = 3, N + 5
    kw = dict(restart=8, maxiter=20, tol=TOL, **CYCLE)
    ref = _singles(mg, H, B, X0, "edges", **kw)

    def padded(A):
        P = np.full((ld, K + 1), POISON, order="F")
        P[:N, :K] = A
        return P
    PB, PX = padded(B), padded(X0)
    dB, dX = ctx.to_device(PB.ravel(order="F")), ctx.to_device(PX.ravel(order="F"))
    its, res, work = H.fgmres_multi_dev(dB, dX, ncols=K, ld=ld, **kw)
    out = dX.download().reshape((ld, K + 1), order="F")
    _assert_columns_equal((out[:N, :K], its, res), ref)
    assert np.all(out[N:, :] == POISON) and np.all(out[:, K] == POISON)
    assert _same(dB.download(), PB.ravel(order="F"))
    assert work == sum(r[1] for r in ref)
    # the argument errors, each raised before X changes
    dX.upload(PX.ravel(order="F"))
    b, x = dB.ptr.value, dX.ptr.value
    He = mg.MeshHierarchy.from_reference(Ho, ctx=ctx, coarse_mode=_lib.COARSE_EXTERNAL)
    bad = [dict(B=None), dict(X=None), dict(H=None), dict(hist=False), dict(its=False), dict(K=0), dict(K=-1),
           dict(ld=N - 1), dict(restart=0), dict(restart=_lib.FGMRES_MAX_RESTART + 1), dict(maxiter=-1), dict(nPre=-1),
           dict(nPost=-1), dict(X=b), dict(X=b + 8 * ld), dict(X=b + 8 * (K - 1) * ld + 8 * (N - 1)), dict(H=He)]
    for a in bad:
        args = dict(H=H, B=b, X=x, K=K, ld=ld)
        args.update(a)
        with pytest.raises(mg.ArgumentError):
            _call(ctx, **args)
        assert _same(dX.download(), PX.ravel(order="F")), a
        assert _same(dB.download(), PB.ravel(order="F")), a
    # fgmres keeps refusing matrices, and says where they go
    with pytest.raises(mg.ArgumentError, match="K right-hand sides"):
        mg.fgmres(H, B, **CYCLE)
    with pytest.raises(mg.ArgumentError, match="fgmres_multi"):
        mg.fgmres(H, mg.DeviceMatrix(ctx, N, 2), **CYCLE)
    # shapes that do not match
    with pytest.raises(mg.DimensionMismatch):
        mg.fgmres_multi(H, B[:-1, :], **CYCLE)
    with pytest.raises(mg.DimensionMismatch):
        mg.fgmres_multi(H, B, X0=X0[:, :2], **CYCLE)


def test_one_level_hierarchy(oracle, mg):
    Ho, _ = oracle.build_dg_agg_hierarchy(16, p=3, pAgg=1, nAgg=2, first=4)
    A = Ho.mStiffness[0]
    H = mg.MeshHierarchy(None, [A], [], [])
    N = A.shape[0]
    B = np.zeros((N, 3), order="F")
    B[:, 0] = oracle.splitmix_normal(N, 1)
    B[:, 2] = oracle.splitmix_normal(N, 2)
    ref = [mg.fgmres(H, B[:, j].copy(), tol=1e-10) for j in range(3)]
    assert [r[1] for r in ref] == [1, 0, 1]
    _assert_columns_equal(mg.fgmres_multi(H, B, tol=1e-10), ref)


# ---- 6. the work space belongs to the context ------------------------------------------------------------------------
def test_fgmres_multi_work_space_lifetime(oracle, mg):
    from agglomerationmultigrid1d_amd import api
    Ho, _ = oracle.build_dg_agg_hierarchy(48, p=3, pAgg=1, nAgg=3, first=4)
    N = Ho.mStiffness[0].shape[0]
    B = np.stack([oracle.splitmix_normal(N, s) for s in (1, 2, 3)], axis=1)
    kw = dict(maxiter=12, tol=1e-8, nPre=2, nPost=1)
    gc.collect()
    start = api.device_memory()
    ctx = mg.Context(0)
    try:
        H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
        built = api.device_memory()[1]
        mg.fgmres_multi(H, B, restart=6, **kw)
        m6 = api.device_memory()[1]
        assert m6 - built >= (2 * 6 + 2) * N * 3 * 8             # the work space (and the cycle's own scratch)
        mg.fgmres_multi(H, B, restart=6, **kw)
        assert api.device_memory()[1] == m6                      # kept, nothing more
        mg.fgmres_multi(H, B, restart=9, **kw)
        assert api.device_memory()[1] - m6 == 2 * 3 * N * 3 * 8  # exchanged for the other size
        mg.fgmres_multi(H, B, restart=2, **kw)
        assert api.device_memory()[1] - m6 == -2 * 4 * N * 3 * 8
        m2 = api.device_memory()[1]
        mg.fgmres_multi(H, B[:, :2], restart=2, **kw)            # fewer columns: another size
        assert api.device_memory()[1] != m2
        H.free()
        for obj in list(H.mSmoothers) + H._ops + H._Ls:
            obj.free()
        gc.collect()
        assert api.device_memory()[1] - start[1] >= (2 * 2 + 2) * N * 2 * 8
    finally:
        ctx.close()
    gc.collect()
    assert api.device_memory() == start
