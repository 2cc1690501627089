"""K-column hybrid / additive element-patch Schwarz sweeps (aggmg_smooth_multi_dev on a smoother of aggmg_patch_schwarz_setup,
patch_sweep_multi_kernel) and the K-column cycle on hybrid patch levels (AGGMG_OPT_PATCH_SCHWARZ_MULTI).

Every column of a K-column run must be BIT FOR BIT the single-column run of that column (compared as uint64 views): the
single-column sweeps are held to the generic route and the float64 model by tests/test_gpu_patch_schwarz.py, so these
comparisons need no tolerance.  One direct comparison against tests/patch_schwarz_model.py at that file's number,
64 eps S max(||u_model||_inf, ||u_0||_inf), keeps "equal to a wrong single run" from passing.

Shapes are the smallest at which the tiling can go wrong (aggmg_patch_schwarz_multi_tile_plan: one slab of 256 / m
elements, 4 S of them halo):

    m   elements per tile   ne    tiles at S = 1        tiles at S = 8
    4   64                  130   3, the last partial   5
    2   128                 270   3                     3

and ne = 2, 3: one and two patches, both ends of the level in one tile.  Operators of the sweep tests are NON-uniform
(patch_schwarz_model.random_block_tridiag): on a uniform operator a wrong patch or column index is invisible; the
dictionary variant needs a uniform one and takes level 0 of uniform.build_device_hierarchy."""
import ctypes

import numpy as np
import pytest

import patch_schwarz_model as pm
from test_gpu_patch_schwarz import EPS, WEIGHTS, sweeps_dev

pytestmark = pytest.mark.gpu

FORMS = [(4, "row"), (2, "row"), (2, "dense")]   # multi_form: compressed couplings with 4 and 2 rows, dense ones with 2
BIG = {4: 130, 2: 270}
KS = (1, 2, 3, 4, 5, 8, 9)        # 9: two groups
KMAX = max(KS)
SWEEPS = (1, 3, 8, 11)            # 11: a chunked run (8 + 3)
CYCLE_KS = (2, 3, 8, 9)
CYCLES = [(3, 3), (2, 1), (0, 2), (1, 0), (11, 1)]


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def _ctx(mg, *opts):
    c = mg.Context(0)
    for o in opts:
        c.set_option(o, 1)
    return c


@pytest.fixture(scope="module")
def ctx_on(mg):
    """a context with AGGMG_OPT_PATCH_SCHWARZ_MULTI on"""
    from agglomerationmultigrid1d_amd import _lib
    return _ctx(mg, _lib.OPT_PATCH_SCHWARZ_MULTI)


@pytest.fixture(scope="module")
def ctx_off(mg):
    return mg.Context(0)


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def plan(mg, m, S, kb):
    """(elements per tile, owned elements of a launch of S sweeps on a group of kb columns, halo, most sweeps per launch)"""
    te, own, halo, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    st = mg.default_context().lib.aggmg_patch_schwarz_multi_tile_plan(int(m), int(S), int(kb), ctypes.byref(te), ctypes.byref(own),
                                                                      ctypes.byref(halo), ctypes.byref(smax))
    assert st == 0
    return te.value, own.value, halo.value, smax.value


def test_the_table_of_shapes(mg):
    tiles = lambda ne, own: -(-ne // own)
    for m, te, ne, t1, t8 in ((4, 64, 130, 3, 5), (2, 128, 270, 3, 3)):
        for kb in (1, 2, 4, 8):
            assert plan(mg, m, 1, kb) == (te, te - 4, 2, 8) and plan(mg, m, 8, kb) == (te, te - 32, 16, 8)
        assert tiles(ne, te - 4) == t1 and tiles(ne, te - 32) == t8
        assert ne % (te - 4) != 0   # the last tile is partial


COLS = 4   # columns one launch of the kernel takes of a group of up to eight (host_plan.hpp: kPatchSchwarzMultiCols)


def launches(K, S, cols=COLS, smax=8):
    """launches of the kernel for S sweeps on K columns: per group of up to 8 columns and chunk of up to smax sweeps one
    launch per `cols` columns"""
    per_chunk = sum(-(-min(8, K - c0) // cols) for c0 in range(0, K, 8))
    return per_chunk * -(-S // smax)


def sweeps_multi(S, U0, B, weights, ld, K, reverse=0):
    """the K-column sweeps through the C entry point on buffers of leading dimension ld with one column more than K, the
    output filled with NaN first: -> (N, K) result; rows past N and the column past K must still be NaN"""
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
    w = np.ascontiguousarray(weights, dtype=np.float64)
    try:
        if reverse is None:   # the Python front end (no direction)
            S.sweeps_multi_dev(dU0, dB, dU, w, ncols=K, ld=ld)
        else:
            c.check(c.lib.aggmg_smooth_multi_dev(c.handle, S.A.handle, S.handle, None if dU0 is None else dU0.ptr, dB.ptr, K, ld,
                                                 w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), int(w.size), int(reverse), dU.ptr))
        out = dU.download().reshape((ld, K + 1), order="F")
    finally:
        for v in (dB, dU0, dU):
            if v is not None:
                v.free()
    assert np.isnan(out[N:, :]).all(), "rows past N were written"
    assert np.isnan(out[:, K]).all(), "a column past K was written"
    return out[:N, :K]


def check_columns(mg, op, S, U0, B, label, model=None, hybrid=True, cols=COLS):
    """every K, ld, first iterate and sweep count against the single-column sweeps of every column, computed once; the
    counter; reverse; the Python front end; (model: the BlockTridiag) column 1 against the float64 model"""
    c = op.ctx
    N = B.shape[0]
    modelled = 0
    for n in SWEEPS:
        ws = WEIGHTS[:n]   # distinct per sweep
        for first in (U0, None):
            R = np.column_stack([sweeps_dev(mg, op, S, None if first is None else first[:, j].copy(), B[:, j].copy(), WEIGHTS, n)
                                 for j in range(KMAX)])
            for K in KS:
                for ld in (N, N + 1):
                    before = c.patch_schwarz_multi_launches()
                    gs_before = c.patch_multi_launches()
                    X = sweeps_multi(S, first, B, ws, ld, K)
                    assert c.patch_schwarz_multi_launches() - before == launches(K, n, cols), (label, K, n)
                    assert c.patch_multi_launches() == gs_before
                    for j in range(K):
                        assert _same(X[:, j], R[:, j]), (label, n, first is not None, K, ld, j, float(np.max(np.abs(X[:, j] - R[:, j]))))
            # the direction means nothing here; the front end's call is the same call
            assert _same(sweeps_multi(S, first, B, ws, N + 1, 3, reverse=1), R[:, :3]), (label, n, "reverse")
            assert _same(sweeps_multi(S, first, B, ws, N, 5, reverse=None), R[:, :5]), (label, n, "front end")
            if model is not None:
                start = np.zeros(N) if first is None else first[:, 1]
                um = model.sweeps(start, B[:, 1], ws, hybrid)
                bound = 64 * EPS * n * max(np.max(np.abs(um)), np.max(np.abs(start)))
                d = float(np.max(np.abs(R[:, 1] - um)))
                print(f"{label} S {n} guess {first is not None}: device-model {d:.3e} bound {bound:.3e}")
                assert d <= bound, (label, n, d, bound)
                modelled += 1
    return modelled


# ---- 1. + 2. sweeps, bit for bit per column against the single-column sweeps, and against the model ---------------------------
@pytest.fixture(scope="module")
def ctx_on_nodict(mg):
    """AGGMG_OPT_PATCH_SCHWARZ_MULTI on, AGGMG_OPT_OPERATOR_DICTIONARY off: the sweeps read the full arrays"""
    from agglomerationmultigrid1d_amd import _lib
    c = _ctx(mg, _lib.OPT_PATCH_SCHWARZ_MULTI)
    c.set_option(_lib.OPT_OPERATOR_DICTIONARY, 0)
    return c


@pytest.mark.parametrize("dictionary", [False, True])
@pytest.mark.parametrize("hybrid", [True, False])
@pytest.mark.parametrize("m,coupling", FORMS)
def test_sweeps_are_single_column_sweeps(mg, ctx_on, ctx_on_nodict, m, coupling, hybrid, dictionary):
    """dictionary True: the default context, which keeps the records of these levels by class although all differ (as many
    classes as elements) -- the DICT kernels on a non-uniform operator; False: the kernels on the full arrays"""
    ctx = ctx_on if dictionary else ctx_on_nodict
    modelled = 0
    for ne in (2, 3, BIG[m]):
        T = pm.random_block_tridiag(m, ne, coupling, 4000 + 10 * ne + m)
        op = mg.DeviceOperator(T.tocsc(), ctx=ctx)
        S = mg.ElementPatchSchwarz(op, m, ne, hybrid=hybrid)
        try:
            assert S.fused and S.width == 2 and S.hybrid == hybrid
            assert (S.dictionary_classes > 0) == dictionary, (ne, S.dictionary_classes)
            N = m * ne
            rng = np.random.default_rng(100 * ne + m)
            U0, B = rng.standard_normal((N, KMAX)), rng.standard_normal((N, KMAX))
            modelled += check_columns(mg, op, S, U0, B, f"m {m} {coupling} hybrid {hybrid} ne {ne} dictionary {dictionary}", T, hybrid)
        finally:
            S.free()
            op.free()
    assert modelled == 3 * len(SWEEPS) * 2


@pytest.mark.parametrize("hybrid", [True, False])
@pytest.mark.parametrize("m,coupling", FORMS)
def test_sweeps_in_launches_of_eight_columns(mg, monkeypatch, m, coupling, hybrid):
    """the KB = 8 instantiations: a context created under AGGMG_PATCH_SCHWARZ_MULTI_COLS=8 (the measurement knob; the default,
    two launches of four per group of eight, is what every other test runs), full arrays and dictionary"""
    from agglomerationmultigrid1d_amd import _lib
    monkeypatch.setenv("AGGMG_PATCH_SCHWARZ_MULTI_COLS", "8")
    ne = BIG[m]
    T = pm.random_block_tridiag(m, ne, coupling, 4100 + m)
    rng = np.random.default_rng(55 + m)
    U0, B = rng.standard_normal((m * ne, KMAX)), rng.standard_normal((m * ne, KMAX))
    for dictionary in (False, True):
        c = _ctx(mg, _lib.OPT_PATCH_SCHWARZ_MULTI)
        c.set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if dictionary else 0)
        op = mg.DeviceOperator(T.tocsc(), ctx=c)
        S = mg.ElementPatchSchwarz(op, m, ne, hybrid=hybrid)
        try:
            assert S.fused and (S.dictionary_classes > 0) == dictionary
            assert check_columns(mg, op, S, U0, B, f"cols 8 m {m} {coupling} hybrid {hybrid} dictionary {dictionary}", T, hybrid, cols=8) == 8
        finally:
            S.free()
            op.free()


# ---- 1. (DICT) a uniform-mesh operator whose smoother has a dictionary, the option on and off -----------------------------------
@pytest.mark.parametrize("p,n", [(3, 144), (1, 272)])   # m = 4: 3 tiles of 64 at S = 1; m = 2: 3 tiles of 128
def test_sweeps_with_the_operator_dictionary(mg, p, n):
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    results = {}
    for on in (True, False):
        c = _ctx(mg, _lib.OPT_PATCH_SCHWARZ_MULTI)
        c.set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
        H = build_device_hierarchy(UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=(4, 2, 2)), c, smoother="patchSchwarz0")
        extra = []
        try:
            op, S = H._ops[0], H.mSmoothers[0]
            m, ne = S.m, S.ne
            assert (m, ne) == (p + 1, n) and S.fused and S.hybrid
            assert (S.dictionary_classes > 0) == on, (on, S.dictionary_classes)
            N = m * ne
            rng = np.random.default_rng(7 + n)
            U0, B = rng.standard_normal((N, KMAX)), rng.standard_normal((N, KMAX))
            check_columns(mg, op, S, U0, B, f"uniform p {p} n {n} dictionary {on}")
            Sa = mg.ElementPatchSchwarz(op, m, ne, hybrid=False)   # the additive form on the same operator
            extra.append(Sa)
            assert (Sa.dictionary_classes > 0) == on
            check_columns(mg, op, Sa, U0, B, f"uniform p {p} n {n} additive dictionary {on}")
            results[on] = [sweeps_multi(X, U0, B, WEIGHTS[:11], N, 9) for X in (S, Sa)]
        finally:
            for x in extra:
                x.free()
            _free_all(H)
    for a, b in zip(results[True], results[False]):
        assert _same(a, b)   # the dictionary's words are the full arrays' words


# ---- 3. the cycle, bit for bit per column, against vcycle_dev ------------------------------------------------------------------
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


@pytest.mark.parametrize("smoother", ["patchSchwarz0", "patchSchwarz"])
@pytest.mark.parametrize("p", [3, 1])
def test_cycle_bitwise_per_column(mg, ctx_on, ctx_off, p, smoother):
    n, ratios = 4608, (4, 2, 2)
    H1, U = _uniform(ctx_on, n, p, ratios, smoother)
    H0, _ = _uniform(ctx_off, n, p, ratios, smoother)
    try:
        N = H1._ops[0].shape[0]
        patch_levels = 1 if smoother == "patchSchwarz0" else len(ratios)
        rng = np.random.default_rng(n + 7 * p)
        B = rng.standard_normal((N, max(CYCLE_KS)))
        X0 = rng.standard_normal((N, max(CYCLE_KS)))
        for K in CYCLE_KS:
            assert H1.multi_info(K) == (True, min(K, 8)), (K, H1.multi_info(K))
            assert H0.multi_info(K) == (False, 1)
        for nPre, nPost in CYCLES:
            # The block-Jacobi levels below the patch level of "patchSchwarz0" qualify by the rule they always had: one fused
            # launch per half-cycle, at most 8 sweeps with the residual -- V(11, 1) on them stays column by column (the same
            # bits, compared below like every other case); on "patchSchwarz" every level chunks its sweeps and runs in groups.
            in_groups = not (smoother == "patchSchwarz0" and nPre + 1 > 8)
            for K in CYCLE_KS:
                assert H1.multi_info(K, nPre, nPost) == ((True, min(K, 8)) if in_groups else (False, 1)), (nPre, nPost, K)
                assert H0.multi_info(K, nPre, nPost) == (False, 1)
            for guess in (X0, None):
                R = _single(H0, guess, B, nPre, nPost)
                for i, K in enumerate(CYCLE_KS):
                    ld = N if i % 2 == 0 else N + 3
                    before = ctx_on.patch_schwarz_multi_launches()
                    X = _multi(H1, None if guess is None else guess[:, :K], B[:, :K], nPre, nPost, ld)
                    want = patch_levels * (launches(K, nPre) + launches(K, nPost)) if in_groups else 0
                    assert ctx_on.patch_schwarz_multi_launches() - before == want, (nPre, nPost, K)
                    for j in range(K):
                        assert _same(X[:, j], R[:, j]), (nPre, nPost, K, j, float(np.max(np.abs(X[:, j] - R[:, j]))))
                # the default context: column by column, the same bits, no launch of the kernel
                X = _multi(H0, None if guess is None else guess[:, :3], B[:, :3], nPre, nPost, N + 3)
                for j in range(3):
                    assert _same(X[:, j], R[:, j]), (nPre, nPost, j)
        assert ctx_off.patch_schwarz_multi_launches() == 0 and ctx_on.patch_multi_launches() == 0
    finally:
        _free_all(H1)
        _free_all(H0)


def test_cycle_with_a_sweep_weight_schedule(mg, ctx_on, ctx_off):
    H1, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchSchwarz0")
    H0, _ = _uniform(ctx_off, 4608, 3, (4, 2, 2), "patchSchwarz0")
    try:
        for H in (H1, H0):
            H.set_sweep_weights(0, [0.9, 0.35, 0.6], [0.8, 0.45, 0.7])
        N = H1._ops[0].shape[0]
        rng = np.random.default_rng(12)
        B, X0 = rng.standard_normal((N, 9)), rng.standard_normal((N, 9))
        assert H1.multi_info(9) == (True, 8) and H0.multi_info(9) == (False, 1)
        R = _single(H0, X0, B, 3, 3)
        before = ctx_on.patch_schwarz_multi_launches()
        X = _multi(H1, X0, B, 3, 3, N + 3)
        assert ctx_on.patch_schwarz_multi_launches() - before == 2 * launches(9, 3) == 6
        for j in range(9):
            assert _same(X[:, j], R[:, j]), j
        H0.clear_sweep_weights()
        assert not _same(_single(H0, X0[:, :1], B[:, :1], 3, 3)[:, 0], R[:, 0])   # the schedule arrives
    finally:
        _free_all(H1)
        _free_all(H0)


def test_with_the_multiplicative_option_on_as_well(mg, ctx_off):
    """options 11 and 14 together: a multiplicative and a hybrid hierarchy each keep their single-column bits, each through
    its own kernel"""
    from agglomerationmultigrid1d_amd import _lib
    c = _ctx(mg, _lib.OPT_PATCH_MULTI, _lib.OPT_PATCH_SCHWARZ_MULTI)
    for smoother in ("patchGS0", "patchSchwarz0"):
        H1, U = _uniform(c, 4608, 3, (4, 2, 2), smoother)
        H0, _ = _uniform(ctx_off, 4608, 3, (4, 2, 2), smoother)
        try:
            N = H1._ops[0].shape[0]
            rng = np.random.default_rng(21)
            B, X0 = rng.standard_normal((N, 9)), rng.standard_normal((N, 9))
            assert H1.multi_info(9) == (True, 8) and H0.multi_info(9) == (False, 1)
            gs, hy = c.patch_multi_launches(), c.patch_schwarz_multi_launches()
            X = _multi(H1, X0, B, 3, 3, N + 1)
            d_gs, d_hy = c.patch_multi_launches() - gs, c.patch_schwarz_multi_launches() - hy
            # (the multiplicative kernel takes a group of eight in one launch, the hybrid one in two of four)
            assert (d_gs, d_hy) == ((4, 0) if smoother == "patchGS0" else (0, 2 * launches(9, 3))), (smoother, d_gs, d_hy)
            R = _single(H0, X0, B, 3, 3)
            for j in range(9):
                assert _same(X[:, j], R[:, j]), (smoother, j)
        finally:
            _free_all(H1)
            _free_all(H0)


# ---- 4. solvers ------------------------------------------------------------------------------------------------------------
def test_solvers_on_matrices(mg, ctx_on):
    K = 3
    H, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchSchwarz0")
    try:
        assert H.multi_info(K) == (True, K)
        b = U.rhs()
        N = len(b)
        rng = np.random.default_rng(5)
        B = np.column_stack([b, rng.standard_normal(N), 3.0 * b + rng.standard_normal(N)])
        X0 = np.column_stack([np.zeros(N), 0.1 * rng.standard_normal(N), rng.standard_normal(N)])
        before = ctx_on.patch_schwarz_multi_launches()
        X, its, res = mg.fgmres_multi(H, B, X0, restart=10, maxiter=40, tol=1e-8)
        assert ctx_on.patch_schwarz_multi_launches() > before
        for j in range(K):
            xs, its0, res0 = mg.fgmres(H, B[:, j].copy(), X0[:, j].copy(), restart=10, maxiter=40, tol=1e-8)
            assert int(its[j]) == its0 and 0 < its0 < 40, (j, its[j], its0)
            assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
            assert list(res[j]) == list(np.atleast_1d(res0)), j
        before = ctx_on.patch_schwarz_multi_launches()
        X, its, res, err = mg.multigrid(H, X0, B, 40, 1e-8, exact=False)
        assert ctx_on.patch_schwarz_multi_launches() > before
        for j in range(K):
            xs, its0, res0, _ = mg.multigrid(H, X0[:, j].copy(), B[:, j].copy(), 40, 1e-8, exact=False)
            assert int(its[j]) == its0 and 0 < its0 < 40, (j, its[j], its0)
            assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
            assert list(res[j]) == list(np.atleast_1d(res0)), j
    finally:
        _free_all(H)


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(mg, ctx_on, ctx_off):
    m, ne, K = 4, 12, 2
    N = m * ne
    T = pm.random_block_tridiag(m, ne, "row", 9)
    w = (ctypes.c_double * 1)(2.0 / 3.0)
    made = []

    def case(c, A, **kw):
        op = mg.DeviceOperator(A, ctx=c)
        S = mg.ElementPatchSchwarz(op, m, ne, **kw)
        bufs = [mg.DeviceMatrix(c, N, K) for _ in range(3)]
        bufs[1].upload(np.ones((N, K)))
        made.extend([S, op] + bufs)
        return op, S, bufs

    def call(c, op, S, u0, b, u, ncols=K, ld=N, nsweeps=1):
        return c.lib.aggmg_smooth_multi_dev(c.handle, op.handle, S.handle, None if u0 is None else u0.ptr, b.ptr, ncols, ld, w, nsweeps, 0, u.ptr)

    try:
        # the option off: the smoother is refused by name, and the message names the option
        op, S, (u0, b, u) = case(ctx_off, T.tocsc())
        with pytest.raises(mg.UnsupportedError) as ei:
            S.sweeps_multi_dev(u0, b, u, [2.0 / 3.0])
        assert "hybrid" in str(ei.value) and "AGGMG_OPT_PATCH_SCHWARZ_MULTI" in str(ei.value), str(ei.value)
        assert ctx_off.patch_schwarz_multi_launches() == 0
        # the option on: the call itself is fine
        op, S, (u0, b, u) = case(ctx_on, T.tocsc())
        before = ctx_on.patch_schwarz_multi_launches()
        S.sweeps_multi_dev(u0, b, u, [2.0 / 3.0])
        assert ctx_on.patch_schwarz_multi_launches() == before + 1
        # argument errors
        for kw in (dict(ld=N - 1), dict(ncols=0), dict(nsweeps=-1), dict(u=u0), dict(u=b)):
            args = dict(u0=u0, b=b, u=u)
            args.update(kw)
            with pytest.raises(mg.ArgumentError):
                ctx_on.check(call(ctx_on, op, S, **args))
        # a form the kernel is not instantiated for: dense couplings with 4 rows per element
        opd, Sd, (u0, b, u) = case(ctx_on, pm.random_block_tridiag(4, ne, "dense", 9).tocsc())
        assert Sd.fused
        with pytest.raises(mg.UnsupportedError) as ei:
            Sd.sweeps_multi_dev(u0, b, u, [2.0 / 3.0])
        assert "4 rows per element" in str(ei.value) and "dense" in str(ei.value), str(ei.value)
        # patches of three elements: the generic route, not the fused one
        op3, S3, (u0, b, u) = case(ctx_on, T.tocsc(), width=3)
        assert not S3.fused and S3.width == 3
        with pytest.raises(mg.UnsupportedError) as ei:
            S3.sweeps_multi_dev(u0, b, u, [2.0 / 3.0])
        assert "generic route" in str(ei.value) and "3 elements" in str(ei.value) and "not the fused" in str(ei.value), str(ei.value)
    finally:
        for x in made:
            x.free()


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(mg, ctx_on):
    m, ne = 4, 130
    T = pm.random_block_tridiag(m, ne, "row", 77)
    op = mg.DeviceOperator(T.tocsc(), ctx=ctx_on)
    S = mg.ElementPatchSchwarz(op, m, ne)
    H, U = _uniform(ctx_on, 4608, 3, (4, 2, 2), "patchSchwarz0")
    try:
        rng = np.random.default_rng(8)
        U0, B = rng.standard_normal((m * ne, 9)), rng.standard_normal((m * ne, 9))
        a, b = (sweeps_multi(S, U0, B, WEIGHTS[:11], m * ne + 1, 9) for _ in range(2))
        assert _same(a, b) and np.isfinite(a).all()
        N = H._ops[0].shape[0]
        X0, Bc = rng.standard_normal((N, 9)), rng.standard_normal((N, 9))
        a, b = (_multi(H, X0, Bc, 3, 3, N) for _ in range(2))
        assert _same(a, b) and np.isfinite(a).all()
    finally:
        S.free()
        op.free()
        _free_all(H)
