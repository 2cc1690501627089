"""K-column multiplicative element-patch sweeps (aggmg_smooth_multi_dev, patch_gs_multi_kernel) and the K-column cycle on
multiplicative patch levels (AGGMG_OPT_PATCH_MULTI).

Every column of a K-column run must be BIT FOR BIT the single-column run of that column: the single-column sweeps are held
to the float64 model by tests/test_gpu_patch_gs.py, so the sweep comparisons need no tolerance.  One direct model
comparison (64 eps S max(||u_model||_inf, ||u_0||_inf), that file's bound) keeps "equal to a wrong single run" from
passing.  Forward single-column sweeps run through aggmg_smooth(_weighted)_dev, reverse ones through the V(0, S)
construction of that file's Case.  Operators of the sweep tests are NON-uniform (patch_schwarz_model.random_block_tridiag):
on a uniform operator a wrong patch or column index is invisible."""
import ctypes
import gc

import numpy as np
import pytest

import patch_gs_model as gm
import patch_schwarz_model as pm
from test_gpu_patch_gs import ALPHA, EPS, SHAPES, WEIGHTS, Case, periodic

pytestmark = pytest.mark.gpu

# the forms the kernel is instantiated for: the couplings set-up stores compressed at m = 2 and 4, and dense at m = 2
FORMS = [(m, c) for m, c in SHAPES if (c == "row" and m in (2, 4)) or (c == "dense" and m == 2)]
KS = (1, 3, 8, 11)
KMAX = max(KS)
CYCLE_KS = (1, 2, 3, 4, 8, 11)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


@pytest.fixture(scope="module")
def ctx_on(mg):
    """a context with AGGMG_OPT_PATCH_MULTI on"""
    from agglomerationmultigrid1d_amd import _lib
    c = mg.Context(0)
    c.set_option(_lib.OPT_PATCH_MULTI, 1)
    return c


@pytest.fixture(scope="module")
def ctx_off(mg):
    return mg.Context(0)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_forms_are_the_three_instantiated():
    assert sorted(FORMS) == [(2, "dense"), (2, "row"), (4, "row")]


def plan(mg, m, S, kb):
    """(elements per tile, owned elements of a launch of S sweeps on a group of kb columns, halo, most sweeps per launch)"""
    te, own, halo, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    st = mg.default_context().lib.aggmg_patch_gs_multi_tile_plan(int(m), int(S), int(kb), ctypes.byref(te), ctypes.byref(own),
                                                                 ctypes.byref(halo), ctypes.byref(smax))
    assert st == 0
    return te.value, own.value, halo.value, smax.value


def group_of(K):
    return 1 if K <= 1 else 2 if K <= 2 else 4 if K <= 4 else 8


def sizes(mg, m, S):
    """2, 3, 5 and the tile boundaries of the launch's plan, over the groups the runs below use"""
    out = {2, 3, 5}
    for kb in (1, 4, 8):
        own = plan(mg, m, S, kb)[1]
        assert own >= 1
        out |= {own - 1, own, own + 1, 2 * own + 1}
    return sorted(x for x in out if x >= 2)


def sweeps_multi(S, U0, B, weights, reverse, ld, K):
    """the K-column sweeps on buffers of leading dimension ld with one column more than K, the output filled with NaN
    first: -> (N, K) result; rows past N and the column past K must still be NaN"""
    c = S.A.ctx
    N = B.shape[0]
    pad = np.zeros((ld, K + 1), order="F")

    def up(A):
        pad[:] = 0.0
        pad[:N, :K] = A[:, :K]
        return c.to_device(pad.ravel(order="F"))

    dB = up(B)
    dU0 = None if U0 is None else up(U0)
    dU = c.to_device(np.full(ld * (K + 1), np.nan))
    try:
        S.sweeps_multi_dev(dU0, dB, dU, weights, reverse=reverse, ncols=K, ld=ld)
        out = dU.download().reshape((ld, K + 1), order="F")
    finally:
        for v in (dB, dU0, dU):
            if v is not None:
                v.free()
    assert np.isnan(out[N:, :]).all(), "rows past N were written"
    assert np.isnan(out[:, K]).all(), "a column past K was written"
    return out[:N, :K]


def weights_of(alpha, n):
    return list(alpha[:n]) if np.ndim(alpha) > 0 else [float(alpha)] * n


# ---- 1. sweeps, bit for bit per column, against the single-column sweeps -------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])   # 1 sweep, 3 sweeps, the most of one launch + 3 (chunked)
@pytest.mark.parametrize("m,coupling", FORMS)
def test_sweeps_are_single_column_sweeps(mg, oracle, m, coupling, which):
    smax = plan(mg, m, 1, 8)[3]
    assert 1 <= smax <= 8
    S = (1, 3, smax + 3)[which]
    modelled = 0
    for ne in sizes(mg, m, min(S, smax)):
        T = pm.random_block_tridiag(m, ne, coupling, 2000 * S + ne)
        C = Case(mg, T)
        try:
            assert C.S.fused and C.S.kind == 3
            N = m * ne
            U0 = np.column_stack([oracle.splitmix_normal(N, 40 + 3 * j + ne) for j in range(KMAX)])
            B = np.column_stack([oracle.splitmix_normal(N, 70 + 5 * j + ne) for j in range(KMAX)])
            for reverse in (False, True):
                for first in (U0, None):
                    for alpha in (ALPHA, WEIGHTS):
                        # the reference, once for all K and ld: the single-column sweeps of every column
                        R = np.column_stack([C.sweeps(None if first is None else first[:, j].copy(), B[:, j].copy(), alpha, S, reverse)
                                             for j in range(KMAX)])
                        ws = weights_of(alpha, S)
                        for K in KS:
                            for ld in (N, N + 3):
                                X = sweeps_multi(C.S, first, B, ws, reverse, ld, K)
                                for j in range(K):
                                    assert _same(X[:, j], R[:, j]), (m, coupling, ne, S, reverse, first is not None, np.ndim(alpha), K, ld, j,
                                                                    float(np.max(np.abs(X[:, j] - R[:, j]))))
                                if K == 3 and ld == N:
                                    # (equal to a WRONG single run cannot pass: column 2 against the float64 model)
                                    start = np.zeros(N) if first is None else first[:, 2]
                                    um = gm.gs_sweeps(T, start, B[:, 2], ws, reverse)
                                    bound = 64 * EPS * S * max(np.max(np.abs(um)), np.max(np.abs(start)))
                                    d = float(np.max(np.abs(X[:, 2] - um)))
                                    print(f"m {m} {coupling} ne {ne} S {S} rev {reverse}: device-model {d:.3e} bound {bound:.3e}")
                                    assert d <= bound
                                    modelled += 1
        finally:
            C.free()
    assert modelled > 0


# ---- 2. dictionary on = off ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dict_ctxs(mg):
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    for on in (True, False):
        out[on] = mg.Context(0)
        out[on].set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
    return out


@pytest.mark.parametrize("m,coupling", FORMS)
def test_dictionary_on_is_dictionary_off(mg, dict_ctxs, m, coupling):
    smax = plan(mg, m, 1, 4)[3]
    own = plan(mg, m, min(3, smax), 4)[1]
    K = 3
    for ne in (5, own + 1, 2 * own + 1):
        T = periodic(m, 3, ne, coupling, 51 + m)
        N = m * ne
        rng = np.random.default_rng(3000 + ne)
        U0, B = rng.standard_normal((N, K)), rng.standard_normal((N, K))
        C = {on: Case(mg, T, ctx=dict_ctxs[on]) for on in (True, False)}
        try:
            assert C[True].S.dictionary_classes > 0
            assert C[False].S.dictionary_classes == 0
            for reverse in (False, True):
                for n in (1, 3, smax + 3):
                    for first in (None, U0):
                        for alpha in (ALPHA, WEIGHTS):
                            ws = weights_of(alpha, n)
                            X1, X0_ = (sweeps_multi(C[on].S, first, B, ws, reverse, N, K) for on in (True, False))
                            assert _same(X1, X0_), (m, coupling, ne, reverse, n, float(np.max(np.abs(X1 - X0_))))
                            start = np.zeros(N) if first is None else first[:, 1]
                            um = gm.gs_sweeps(T, start, B[:, 1], ws, reverse)
                            assert np.max(np.abs(X1[:, 1] - um)) <= 64 * EPS * n * max(np.max(np.abs(um)), np.max(np.abs(start)))
        finally:
            for on in (True, False):
                C[on].free()


# ---- 3. the cycle, bit for bit per column, against vcycle_dev --------------------------------------------------------------
def _uniform(ctx, n, p, ratios, smoother):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios)
    return build_device_hierarchy(U, ctx, smoother=smoother), U


def _free_all(H):
    sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
    H.free()
    for x in sms + ops + Ls:
        x.free()


def _single(H, X0, B, nPre, nPost):
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


def _multi(H, X0, B, nPre, nPost, ld):
    """K-column device cycle on column-major buffers with leading dimension ld, the output filled with NaN first"""
    c = H.ctx
    N, K = B.shape
    pad = np.zeros((ld, K), order="F")

    def up(A):
        pad[:] = 0.0
        pad[:N] = A
        return c.to_device(pad.ravel(order="F"))

    dB = up(B)
    dX0 = None if X0 is None else up(X0)
    dX = c.to_device(np.full(ld * K, np.nan))
    H.vcycle_multi_dev(dX0, dB, dX, K, ld, nPre, nPost)
    out = dX.download().reshape((ld, K), order="F")
    assert np.isnan(out[N:]).all()
    return out[:N]


@pytest.mark.parametrize("smoother", ["patchGS0", "patchGS"])
@pytest.mark.parametrize("ratios", [(4, 2, 2), (2, 2, 2, 2)])
@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("n", [64, 4608])
def test_cycle_bitwise_per_column(mg, ctx_on, ctx_off, n, p, ratios, smoother):
    H1, U = _uniform(ctx_on, n, p, ratios, smoother)
    H0, _ = _uniform(ctx_off, n, p, ratios, smoother)
    try:
        N = H1._ops[0].shape[0]
        rng = np.random.default_rng(n + 7 * p + sum(ratios))
        B = rng.standard_normal((N, max(CYCLE_KS)))
        X0 = rng.standard_normal((N, max(CYCLE_KS)))
        sweeps = [(3, 3), (1, 2), (0, 2), (2, 0)] + ([(9, 1)] if n == 64 else [])   # (9, 1): more than one launch takes
        for nPre, nPost in sweeps:
            # In groups wherever every level qualifies.  The block-Jacobi levels below the patch level of "patchGS0" qualify
            # by the rule they had before the option: one fused launch per half-cycle, which takes at most 8 sweeps with the
            # residual -- V(9, 1) on them stays column by column (the same bits, compared below like every other case); on
            # "patchGS" every level chunks its sweeps and V(9, 1) runs in groups.
            in_groups = not (smoother == "patchGS0" and nPre + 1 > 8)
            for K in CYCLE_KS:
                fused, group = H1.multi_info(K, nPre, nPost)
                if in_groups:
                    assert fused and 1 <= group <= K, (nPre, nPost, K, fused, group)
                else:
                    assert (fused, group) == (False, 1), (nPre, nPost, K, fused, group)
                assert H0.multi_info(K, nPre, nPost) == (False, 1)
            for guess in (X0, None):
                R = _single(H0, guess, B, nPre, nPost)
                for i, K in enumerate(CYCLE_KS):
                    ld = N if i % 2 == 0 else N + 3
                    X = _multi(H1, None if guess is None else guess[:, :K], B[:, :K], nPre, nPost, ld)
                    for j in range(K):
                        assert _same(X[:, j], R[:, j]), (nPre, nPost, K, j, float(np.max(np.abs(X[:, j] - R[:, j]))))
                # the default context: column by column, the same bits
                X = _multi(H0, None if guess is None else guess[:, :3], B[:, :3], nPre, nPost, N + 3)
                for j in range(3):
                    assert _same(X[:, j], R[:, j]), (nPre, nPost, j)
    finally:
        _free_all(H1)
        _free_all(H0)


def test_cycle_with_a_sweep_weight_schedule(mg, ctx_on, ctx_off):
    H1, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchGS0")
    H0, _ = _uniform(ctx_off, 4608, 3, (4, 2, 2), "patchGS0")
    try:
        for H in (H1, H0):
            H.set_sweep_weights(0, [0.9, 0.35, 0.6], [0.8, 0.45, 0.7])
        N = H1._ops[0].shape[0]
        rng = np.random.default_rng(12)
        B, X0 = rng.standard_normal((N, 11)), rng.standard_normal((N, 11))
        assert H1.multi_info(11)[0] and H0.multi_info(11) == (False, 1)
        R = _single(H0, X0, B, 3, 3)
        X = _multi(H1, X0, B, 3, 3, N + 3)
        for j in range(11):
            assert _same(X[:, j], R[:, j]), j
        H0.clear_sweep_weights()
        assert not _same(_single(H0, X0[:, :1], B[:, :1], 3, 3)[:, 0], R[:, 0])   # the schedule arrives
    finally:
        _free_all(H1)
        _free_all(H0)


# ---- 4. against the oracle ----------------------------------------------------------------------------------------------
def test_against_oracle(mg, ctx_on, oracle):
    """every column against the reference's cycle with the model smoother on level 0, at the bar of
    tests/test_gpu_multi_rhs.py: ||A (x_j - x_ref,j)|| <= 1e-12 (||b_j|| + ||A x0_j||)"""
    Ho, b = oracle.build_dg_agg_hierarchy(64, p=3, pAgg=1, nAgg=3, first=4)
    Hm = gm.with_gs_smoothers(oracle, Ho, [0])
    ops = [mg.DeviceOperator(A, ctx=ctx_on) for A in Ho.mStiffness]
    m, ne = pm.level_shape(Ho, 0)
    sms = [mg.ElementPatchGaussSeidel(ops[0], m, ne)] + [Ho.mSmoothers[k] for k in range(1, len(ops) - 1)]
    H = mg.MeshHierarchy(Ho.mMeshes, ops, sms, Ho.mInterpolation, ctx=ctx_on)
    try:
        fused, group = H.multi_info(4)
        assert fused and group == 4
        N = len(b)
        rng = np.random.default_rng(3)
        B = np.column_stack([b] + [rng.standard_normal(N) for _ in range(3)])
        X0 = np.column_stack([np.zeros(N)] + [rng.standard_normal(N) for _ in range(3)])
        before = ctx_on.patch_multi_launches()
        X = mg.multigrid_v_cycle(H, X0, B)
        assert ctx_on.patch_multi_launches() == before + 2
        A = Ho.mStiffness[0]
        for j in range(4):
            xr = oracle.multigrid_v_cycle(Hm, X0[:, j].copy(), B[:, j].copy(), 3, 3, ALPHA)
            scale = np.linalg.norm(B[:, j]) + np.linalg.norm(A @ X0[:, j])
            d = np.linalg.norm(A @ (X[:, j] - xr))
            print(f"column {j}: ||A (x - x_ref)|| = {d:.3e}, bound {1e-12 * scale:.3e}")
            assert d <= 1e-12 * scale, j
    finally:
        H.free()


# ---- 5. solvers ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver_case(mg, ctx_on):
    H, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchGS0")
    b = U.rhs()
    N = len(b)
    u_star, it, _, _ = mg.multigrid(H, np.zeros(N), b, 40, 1e-13, exact=False)
    assert np.isfinite(u_star).all()
    noise = np.random.default_rng(5).standard_normal(N) * np.max(np.abs(u_star))
    yield dict(H=H, b=b, N=N, u_star=u_star, noise=noise)
    _free_all(H)


@pytest.mark.parametrize("K", [3, 8])
def test_solvers_on_matrices(mg, solver_case, K):
    d = solver_case
    H, N = d["H"], d["N"]
    assert H.multi_info(K)[0]
    X0 = np.column_stack([d["u_star"] + 10.0 ** (-2 * j) * d["noise"] for j in range(K)])
    B = np.column_stack([d["b"]] * K)
    before = H.ctx.patch_multi_launches()
    X, its, res, err = mg.multigrid(H, X0, B, 40, 1e-9, exact=False)
    assert H.ctx.patch_multi_launches() > before
    counts = []
    for j in range(K):
        xs, its0, res0, _ = mg.multigrid(H, X0[:, j].copy(), B[:, j].copy(), 40, 1e-9, exact=False)
        assert int(its[j]) == its0, (j, its[j], its0)
        assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
        assert list(res[j]) == list(np.atleast_1d(res0)), j
        counts.append(its0)
    assert len(set(counts)) >= 2 and max(counts) < 40, counts   # right-hand sides that finish at different cycles
    X, its, res = mg.pcg(H, B, X0, maxiter=40, tol=1e-9)
    counts = []
    for j in range(K):
        xs, its0, res0 = mg.pcg(H, B[:, j].copy(), X0[:, j].copy(), maxiter=40, tol=1e-9)
        assert int(its[j]) == its0, (j, its[j], its0)
        assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
        assert list(res[j]) == list(np.atleast_1d(res0)), j
        counts.append(its0)
    assert len(set(counts)) >= 2 and max(counts) < 40, counts


# ---- 6. launch count -------------------------------------------------------------------------------------------------------
def test_launch_count(mg, ctx_on, ctx_off):
    K = 11
    for ctx in (ctx_on, ctx_off):
        H, U = _uniform(ctx, 4608, 3, (4, 2, 2), "patchGS0")
        try:
            N = H._ops[0].shape[0]
            fused, group = H.multi_info(K)
            B = np.random.default_rng(1).standard_normal((N, K))
            before = ctx.patch_multi_launches()
            _multi(H, None, B, 3, 3, N)
            ctx.synchronize()
            if ctx is ctx_on:
                assert fused
                assert ctx.patch_multi_launches() - before == 2 * -(-K // group)
            else:
                assert (fused, group) == (False, 1)
                assert ctx.patch_multi_launches() == 0
        finally:
            _free_all(H)


# ---- 7. coverage and refusals ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["patchSchwarz0", "blockGS"])
def test_other_smoothers_stay_column_by_column(mg, ctx_on, smoother):
    H, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), smoother)
    try:
        assert H.multi_info(3) == (False, 1)
        N = H._ops[0].shape[0]
        rng = np.random.default_rng(4)
        B, X0 = rng.standard_normal((N, 3)), rng.standard_normal((N, 3))
        for guess in (X0, None):
            R = _single(H, guess, B, 3, 3)
            X = _multi(H, guess, B, 3, 3, N + 1)
            for j in range(3):
                assert _same(X[:, j], R[:, j]), j
    finally:
        _free_all(H)


def test_refusals(mg):
    c = mg.default_context()
    m, ne, K = 4, 12, 2
    T = pm.random_block_tridiag(m, ne, "row", 9)
    N = m * ne
    op = mg.DeviceOperator(T.tocsc())
    G = mg.ElementPatchGaussSeidel(op, m, ne)
    dB, dU0, dU = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
    dB.upload(np.ones((N, K)))
    G.sweeps_multi_dev(dU0, dB, dU, [ALPHA])   # the call itself is fine
    # smoothers outside the coverage: UnsupportedError naming the reason
    Hy = mg.ElementPatchSchwarz(op, m, ne)
    BJ = mg.BlockJacobi(op, mg.element_patch_lists(m, ne, 1))
    w = (ctypes.c_double * 1)(ALPHA)

    def call(S, u0=dU0, b=dB, u=dU, ncols=K, ld=N, nsweeps=1):
        return c.lib.aggmg_smooth_multi_dev(c.handle, op.handle, S.handle, None if u0 is None else u0.ptr, b.ptr, ncols, ld, w, nsweeps, 0,
                                            u.ptr)

    for S, word in ((Hy, "hybrid"), (BJ, "not a fused element-patch smoother")):
        with pytest.raises(mg.UnsupportedError) as ei:
            c.check(call(S))
        assert word in str(ei.value), str(ei.value)
    # a form the kernel is not instantiated for: dense couplings with 4 rows per element
    Td = pm.random_block_tridiag(4, ne, "dense", 9)
    opd = mg.DeviceOperator(Td.tocsc())
    Gd = mg.ElementPatchGaussSeidel(opd, 4, ne)
    with pytest.raises(mg.UnsupportedError) as ei:
        Gd.sweeps_multi_dev(dU0, dB, dU, [ALPHA])
    assert "4 rows per element" in str(ei.value) and "dense" in str(ei.value)
    # argument errors
    for kw in (dict(ld=N - 1), dict(ncols=0), dict(nsweeps=-1), dict(u=dU0), dict(u=dB)):
        with pytest.raises(mg.ArgumentError):
            c.check(call(G, **kw))
    for x in (G, Hy, BJ, Gd, op, opd, dB, dU0, dU):
        x.free()


# ---- 8. memory -------------------------------------------------------------------------------------------------------------
def test_memory_returns(mg, ctx_on):
    from agglomerationmultigrid1d_amd.api import device_memory

    def round_trip():
        H, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchGS")
        N = H._ops[0].shape[0]
        assert H.multi_info(11)[0]
        B = np.random.default_rng(2).standard_normal((N, 11))
        held = device_memory()[1]
        _multi(H, None, B, 9, 9, N)   # (chunked sweeps: the patch levels' second vectors in use)
        grown = device_memory()[1]
        _free_all(H)
        return held, grown

    round_trip()   # (the context's own work vectors grow on first use and stay)
    gc.collect()
    ctx_on.synchronize()
    start = device_memory()
    held, grown = round_trip()
    assert grown > held > start[1]
    gc.collect()
    ctx_on.synchronize()
    assert device_memory() == start
