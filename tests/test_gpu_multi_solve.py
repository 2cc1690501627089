"""K right-hand sides through the outer loops (EXTENSION: the reference's solvers take vectors, src/solvers.jl:116-139):
aggmg_residual_multi_dev, aggmg_dot_cols_dev / aggmg_norm2_cols_dev, aggmg_pcg_multi_dev, aggmg_multigrid_multi_dev and
their Python surfaces (pcg / multigrid on 2-D arrays and DeviceMatrix).  The contract is bitwise: column j of every result
-- residual, dot, norm, iterate, iteration count, residual / error history -- is what the single-vector entry point gives on
column j (multigrid's histories: those of its AGGMG_OPT_MG_CHECKPOINT = 0 form; against the default form the iterates are
bit-equal and the histories agree to the tolerances tests/test_gpu_solvers.py uses between the two single-column forms).

The solver tests make the columns finish at different iterations on purpose (X0[:, j] = u* + 10^(-2j) noise, u* from a long
run, tol 3.5 decades above where the long run's history stalls), so that columns leave the active set one after another and
the compaction is exercised: they assert at least three distinct single-column iteration counts.  The spread of the
multigrid inputs was checked with the CPU oracle's multigrid beforehand (ne = 256: 135, 105, 75, 46, 23, 7, 1, ... cycles).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 8, 11)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    return mg.Context(0)


def _uniform(mg, ctx, n, p, ratios, **kw):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios)
    return build_device_hierarchy(U, ctx, **kw), U


def _upload(ctx, A, ld):
    """(N, K) host array -> column-major device buffer with leading dimension ld (the padding rows hold NaN)"""
    N, K = A.shape
    pad = np.full((ld, K), np.nan, order="F")
    pad[:N] = A
    return ctx.to_device(pad.ravel(order="F"))


def _download(d, N, K, ld):
    return d.download().reshape((ld, K), order="F")[:N]


def _residual_single(ctx, op, x, b):
    N = op.shape[0]
    dx, db, dr = ctx.to_device(x), ctx.to_device(b), ctx.alloc(N)
    ctx.check(ctx.lib.aggmg_residual_dev(ctx.handle, op.handle, dx.ptr, db.ptr, dr.ptr))
    return dr.download()


def _check_residual(mg, ctx, op, seed):
    N = op.shape[0]
    rng = np.random.default_rng(seed)
    Kmax = max(KS)
    X, B = rng.standard_normal((N, Kmax)), rng.standard_normal((N, Kmax))
    ref = np.column_stack([_residual_single(ctx, op, X[:, j], B[:, j]) for j in range(Kmax)])
    ref0 = np.column_stack([_residual_single(ctx, op, X[:, j], np.zeros(N)) for j in range(Kmax)])
    for i, K in enumerate(KS):
        ld = N if i % 2 == 0 else N + 3
        dX, dB = _upload(ctx, X[:, :K], ld), _upload(ctx, B[:, :K], ld)
        dR = ctx.to_device(np.full(ld * K, np.nan))
        op.residual_multi_dev(dX, dB, dR, K, ld)
        R = _download(dR, N, K, ld)
        for j in range(K):
            assert np.array_equal(R[:, j], ref[:, j]), (K, ld, j, float(np.max(np.abs(R[:, j] - ref[:, j]))))
        if ld > N:      # the rows between the columns are left alone
            assert np.isnan(dR.download().reshape((ld, K), order="F")[N:]).all()
        # no right-hand side: the bits of a zero matrix
        dR0 = ctx.to_device(np.full(ld * K, np.nan))
        op.residual_multi_dev(dX, None, dR0, K, ld)
        R0 = _download(dR0, N, K, ld)
        for j in range(K):
            assert np.array_equal(R0[:, j], ref0[:, j]), (K, ld, j)


@pytest.mark.parametrize("p", [1, 3])
@pytest.mark.parametrize("ratios", [(4, 2, 2), (2, 2, 2, 2)])
@pytest.mark.parametrize("n", [64, 4608, 2**15])
def test_residual_bitwise_per_column(mg, ctx, n, p, ratios):
    """the fine operator (compressed couplings, M = p + 1) and the first agglomerated level's (dense, M = 2)"""
    H, U = _uniform(mg, ctx, n, p, ratios)
    for level in (0, 1):
        op = H._ops[level]
        r, w = op.residual_multi_launch_bytes(1)          # the K-column kernel covers the operator
        assert r > 0 and w == 8 * op.shape[0]
        _check_residual(mg, ctx, op, n + 7 * p + sum(ratios) + level)
    H.free()


def test_residual_fallback_cg_chain(mg, ctx, oracle):
    from agglomerationmultigrid1d_amd import _lib
    Ho, b = oracle.build_cg_hierarchy(256, ps=(4, 2, 1), nDG=1, pDG=0)
    H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
    op = H._ops[0]
    with pytest.raises(_lib.UnsupportedError):
        op.residual_multi_launch_bytes(3)                 # column by column
    _check_residual(mg, ctx, op, 5)
    H.free()


def test_residual_byte_model(mg, ctx):
    H, U = _uniform(mg, ctx, 4096, 3, (4, 2, 2))
    for level in (0, 1):
        op = H._ops[level]
        N = op.shape[0]
        r1, w1 = op.residual_multi_launch_bytes(1)
        for K in (2, 8, 11):
            assert op.residual_multi_launch_bytes(K) == (r1 + (K - 1) * 16 * N, K * 8 * N)
            assert op.residual_multi_launch_bytes(K, has_b=False) == (r1 + (K - 1) * 16 * N - K * 8 * N, K * 8 * N)
    H.free()


@pytest.mark.parametrize("n", [1, 255, 1024 * 256 + 5])
def test_column_dots_and_norms(mg, ctx, n):
    rng = np.random.default_rng(n)
    for K, ld in ((1, n), (5, n + 3), (11, n)):
        X, Y = rng.standard_normal((n, K)), rng.standard_normal((n, K))
        dX, dY = _upload(ctx, X, ld), _upload(ctx, Y, ld)
        d = ctx.dot_cols(dX, dY, n, K, ld)
        nr = ctx.norm2_cols(dX, n, K, ld)
        assert d.shape == (K,) and nr.shape == (K,)
        for j in range(K):
            dx, dy = ctx.to_device(X[:, j]), ctx.to_device(Y[:, j])
            assert d[j] == mg.dot(dx, dy), (K, j)
            assert nr[j] == mg.norm2(dx), (K, j)
    M = mg.DeviceMatrix(ctx, n, 3)
    A = rng.standard_normal((n, 3))
    M.upload(A)
    assert np.array_equal(ctx.norm2_cols(M), [mg.norm2(ctx.to_device(A[:, j])) for j in range(3)])
    assert np.array_equal(ctx.dot_cols(M, M), [mg.dot(ctx.to_device(A[:, j]), ctx.to_device(A[:, j])) for j in range(3)])


# ---- the solvers ---------------------------------------------------------------------------------------------------
def _contexts(mg):
    """(default context, one with AGGMG_OPT_MG_CHECKPOINT = 0: multigrid's form with a residual launch of its own)"""
    from agglomerationmultigrid1d_amd import _lib
    c1, c0 = mg.Context(0), mg.Context(0)
    c0.set_option(_lib.OPT_MG_CHECKPOINT, 0)
    return c1, c0


def _staggered_guesses(u_star, noise, K):
    return np.column_stack([u_star + 10.0 ** (-2 * j) * noise for j in range(K)])


def _stall(hist, nb):
    """where a long run's history stalls, relative to ||b||; never below the fp64 rounding of a residual"""
    return max(float(np.nanmin(hist)) / nb, np.finfo(float).eps)


@pytest.fixture(scope="module")
def dg_case(mg, oracle):
    """DG p = 3, 256 elements, three agglomerated levels (the K-column launches cover it), its right-hand side, u* from long
    single-vector runs, and the noise of the staggered initial guesses"""
    Ho, b = oracle.build_dg_agg_hierarchy(256, p=3, pAgg=1, nAgg=3, first=4)
    c1, c0 = _contexts(mg)
    H1, H0 = mg.MeshHierarchy.from_reference(Ho, ctx=c1), mg.MeshHierarchy.from_reference(Ho, ctx=c0)
    assert H1.multi_info(4)[0] and H0.multi_info(4)[0]
    N = len(b)
    nb = np.linalg.norm(b)
    u_mg, _, long_mg, _ = mg.multigrid(H0, np.zeros(N), b, 600, 0.0, exact=False)
    _, _, long_cg = mg.pcg(H0, b, maxiter=60, tol=0.0)
    assert np.isfinite(u_mg).all()
    return dict(H1=H1, H0=H0, b=b, N=N, nb=nb, u_mg=u_mg, u_cg=u_mg, noise=oracle.splitmix_normal(N, 17),
                tol_mg=10.0 ** 3.5 * _stall(long_mg, nb), tol_cg=10.0 ** 3.5 * _stall(long_cg, nb))


def _assert_multigrid_columns(mg, H1, H0, X0, B, maxiter, tol, exact, check_every, want_spread=False):
    N, K = B.shape
    X, its, res, err = mg.multigrid(H1, X0, B, maxiter, tol, exact=exact, check_every=check_every)
    assert X.shape == (N, K) and len(its) == K and len(res) == K and len(err) == K
    counts = []
    for j in range(K):
        x0, b = X0[:, j].copy(), B[:, j].copy()
        xs, its0, res0, err0 = mg.multigrid(H0, x0, b, maxiter, tol, exact=exact, check_every=check_every)
        assert int(its[j]) == its0, (j, its[j], its0)
        assert np.array_equal(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
        assert res[j] == res0, j                                       # bit for bit: the checkpoint-free form
        assert err[j] == err0, j
        xc, itc, resc, errc = mg.multigrid(H1, x0, b, maxiter, tol, exact=exact, check_every=check_every)
        assert int(its[j]) == itc and np.array_equal(X[:, j], xc), j   # the default (checkpoint) form: the same iterates
        assert len(resc) == len(res[j]) and len(errc) == len(err[j])
        assert np.allclose(res[j], resc, rtol=1e-10, atol=1e-13 * np.linalg.norm(b))
        assert np.allclose(err[j], errc, rtol=1e-9, atol=1e-14)
        counts.append(its0)
    if want_spread:
        assert len(set(counts)) >= 3, counts      # otherwise the compaction path has not been exercised
    return counts


@pytest.mark.parametrize("K", [1, 3, 8, 11])
def test_multigrid_on_matrices(mg, dg_case, K):
    d = dg_case
    X0 = _staggered_guesses(d["u_mg"], d["noise"], K)
    B = np.column_stack([d["b"]] * K)
    spread = K >= 8
    counts = _assert_multigrid_columns(mg, d["H1"], d["H0"], X0, B, 200, d["tol_mg"], True, 1, want_spread=spread)
    if spread:
        assert max(counts) < 200                  # every column converges here
    # some columns do not converge; the others leave early
    counts = _assert_multigrid_columns(mg, d["H1"], d["H0"], X0, B, 30, d["tol_mg"], False, 1)
    if spread:
        assert counts.count(30) >= 2 and min(counts) < 30
    _assert_multigrid_columns(mg, d["H1"], d["H0"], X0, B, 40, d["tol_mg"], K == 3, 3)     # check_every = 3
    _assert_multigrid_columns(mg, d["H1"], d["H0"], X0, B, 7, 1e-30, False, 3)             # 7 = 3 + 3 + 1 cycles
    # maxiter = 0: zeros, no checks
    X, its, res, err = mg.multigrid(d["H1"], X0, B, 0, 1e-10, exact=False)
    assert not X.any() and not np.any(its) and res == [[]] * K and err == [[]] * K


@pytest.mark.parametrize("K", [8, 11])
def test_multigrid_work_follows_the_active_columns(mg, dg_case, K):
    d = dg_case
    H = d["H1"]
    c = H.ctx
    N = d["N"]
    X0 = _staggered_guesses(d["u_mg"], d["noise"], K)
    dX0, dB, dX = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
    dX0.upload(X0)
    dB.upload(np.column_stack([d["b"]] * K))
    for ce in (1, 3):
        ncyc, res, err, work = H.multigrid_multi_dev(dX0, dB, dX, 200, d["tol_mg"], check_every=ce)
        assert len(set(ncyc.tolist())) >= 3, ncyc
        assert K <= work <= int(np.sum(ncyc + 1)), (work, ncyc)
        assert work == int(np.sum(ncyc))                      # a finished column runs no further cycle
        assert work < K * int(np.max(ncyc))


@pytest.mark.parametrize("K", [1, 3, 8, 11])
def test_pcg_on_matrices(mg, dg_case, K):
    d = dg_case
    H = d["H1"]
    N = d["N"]
    X0 = _staggered_guesses(d["u_cg"], d["noise"], K)
    B = np.column_stack([d["b"]] * K)
    for maxiter, tol in ((100, d["tol_cg"]), (6, d["tol_cg"]), (0, 1e-10)):
        X, its, res = mg.pcg(H, B, X0, maxiter=maxiter, tol=tol)
        assert X.shape == (N, K) and len(its) == K and len(res) == K
        counts = []
        for j in range(K):
            xs, its0, res0 = mg.pcg(H, B[:, j].copy(), X0[:, j].copy(), maxiter=maxiter, tol=tol)
            assert int(its[j]) == its0, (j, its[j], its0)
            assert np.array_equal(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
            assert res[j] == res0, j
            counts.append(its0)
        if K >= 8 and maxiter == 100:
            assert len(set(counts)) >= 3, counts  # otherwise the compaction path has not been exercised
            assert max(counts) < 100
        if K >= 8 and maxiter == 6:
            assert counts.count(6) >= 2 and min(counts) < 6, counts   # some columns do not converge
        if maxiter == 0:
            assert np.array_equal(X, X0) and res == [[]] * K
    # zero guesses: X0 = None
    X, its, res = mg.pcg(H, B[:, :K], maxiter=4, tol=1e-30)
    xs, its0, res0 = mg.pcg(H, d["b"], maxiter=4, tol=1e-30)
    for j in range(K):
        assert np.array_equal(X[:, j], xs) and int(its[j]) == its0 and res[j] == res0


@pytest.mark.parametrize("K", [8, 11])
def test_pcg_work_follows_the_active_columns(mg, dg_case, K):
    d = dg_case
    H = d["H1"]
    c = H.ctx
    N = d["N"]
    dB, dX = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
    dB.upload(np.column_stack([d["b"]] * K))
    dX.upload(_staggered_guesses(d["u_cg"], d["noise"], K))
    its, res, work = H.pcg_multi_dev(dB, dX, maxiter=100, tol=d["tol_cg"])
    assert len(set(its.tolist())) >= 3, its
    assert K <= work <= int(np.sum(its + 1)), (work, its)
    assert work < K * (int(np.max(its)) + 1)
    # device matrices through the public function: the result stays on the device, X0 is left alone
    dX0 = mg.DeviceMatrix(c, N, K)
    X0 = _staggered_guesses(d["u_cg"], d["noise"], K)
    dX0.upload(X0)
    Xd, its2, res2 = mg.pcg(H, dB, dX0, maxiter=100, tol=d["tol_cg"])
    assert isinstance(Xd, mg.DeviceMatrix) and np.array_equal(its2, its) and res2 == res
    assert np.array_equal(Xd.download(), dX.download()) and np.array_equal(dX0.download(), X0)


def test_solvers_on_a_multi_tile_hierarchy(mg):
    """uniform generator, 4608 elements (75 K-column tiles on the fine level), distinct right-hand sides, ld = N"""
    c1, c0 = _contexts(mg)
    H1, U = _uniform(mg, c1, 4608, 3, (4, 2, 2))
    H0, _ = _uniform(mg, c0, 4608, 3, (4, 2, 2))
    assert H1.multi_info(8)[0]
    b = U.rhs()
    N, K = len(b), 8
    rng = np.random.default_rng(8)
    B = np.column_stack([b * (1.0 + j) if j % 2 == 0 else rng.standard_normal(N) for j in range(K)])
    X0 = rng.standard_normal((N, K)) * (10.0 ** -np.arange(K))
    _assert_multigrid_columns(mg, H1, H0, X0, B, 12, 1e-3, False, 1)
    _assert_multigrid_columns(mg, H1, H0, X0, B, 5, 1e-30, False, 2)
    X, its, res = mg.pcg(H1, B, X0, maxiter=12, tol=1e-6)
    for j in range(K):
        xs, its0, res0 = mg.pcg(H1, B[:, j].copy(), X0[:, j].copy(), maxiter=12, tol=1e-6)
        assert int(its[j]) == its0 and res[j] == res0 and np.array_equal(X[:, j], xs), j
    H1.free()
    H0.free()


def test_solvers_column_by_column_fallback(mg, oracle):
    """a hierarchy the K-column cycle does not cover (CG chain levels: fused = 0), the same contract"""
    Ho, b = oracle.build_cg_hierarchy(256, ps=(4, 2, 1), nDG=1, pDG=0)
    c1, c0 = _contexts(mg)
    H1, H0 = mg.MeshHierarchy.from_reference(Ho, ctx=c1), mg.MeshHierarchy.from_reference(Ho, ctx=c0)
    K = 3
    assert H1.multi_info(K) == (False, 1)
    N = len(b)
    rng = np.random.default_rng(2)
    B = np.column_stack([b, 2.0 * b, rng.standard_normal(N)])
    X0 = rng.standard_normal((N, K)) * np.array([1.0, 1e-3, 1e-6])
    _assert_multigrid_columns(mg, H1, H0, X0, B, 25, 1e-5, False, 1)
    _assert_multigrid_columns(mg, H1, H0, X0, B, 10, 1e-30, False, 3)
    X, its, res = mg.pcg(H1, B, X0, maxiter=15, tol=1e-8)
    for j in range(K):
        xs, its0, res0 = mg.pcg(H1, B[:, j].copy(), X0[:, j].copy(), maxiter=15, tol=1e-8)
        assert int(its[j]) == its0 and res[j] == res0 and np.array_equal(X[:, j], xs), j


def test_leading_dimension_and_raw_buffers(mg, dg_case):
    """ld = N + 3 through the device entry points: the same columns, the rows between them untouched"""
    d = dg_case
    H = d["H1"]
    c = H.ctx
    N, K, ld = d["N"], 5, d["N"] + 3
    X0 = _staggered_guesses(d["u_cg"], d["noise"], K)
    B = np.column_stack([d["b"]] * K)
    Xr, itr, resr = mg.pcg(H, B, X0, maxiter=100, tol=d["tol_cg"])
    dB, dX = _upload(c, B, ld), _upload(c, X0, ld)
    its, res, _ = H.pcg_multi_dev(dB, dX, K, ld, maxiter=100, tol=d["tol_cg"])
    got = dX.download().reshape((ld, K), order="F")
    assert np.array_equal(got[:N], Xr) and np.isnan(got[N:]).all()
    assert np.array_equal(its, itr) and res == resr
    Xm, itm, resm, _ = mg.multigrid(H, X0, B, 60, d["tol_mg"], exact=False)
    dX0, dXo = _upload(c, X0, ld), c.to_device(np.full(ld * K, np.nan))
    ncyc, res, err, _ = H.multigrid_multi_dev(dX0, dB, dXo, 60, d["tol_mg"], K, ld)
    got = dXo.download().reshape((ld, K), order="F")
    assert np.array_equal(got[:N], Xm) and np.isnan(got[N:]).all()
    assert np.array_equal(ncyc, itm) and res == resm and err == [[]] * K


def test_argument_errors(mg, dg_case, oracle):
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.api import ArgumentError, DimensionMismatch
    d = dg_case
    H = d["H1"]
    c = H.ctx
    N, K = d["N"], 3
    op = H._ops[0]
    dA, dB, dC = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
    # residual
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(None, dB, dC, K, N)            # NULL X
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(dA, dB, None, K, N)            # NULL R
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(dA, dB, dC, K, N - 1)          # ld < N
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(dA, dB, dC, 0, N)              # no columns
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(dA, dB, dA)                    # R is X
    with pytest.raises(ArgumentError):
        op.residual_multi_dev(dA, dB, dB)                    # R is B
    with pytest.raises(DimensionMismatch):
        op.residual_multi_dev(dA, dB, mg.DeviceMatrix(c, N, K - 1))
    # dots
    with pytest.raises(ArgumentError):
        c.dot_cols(dA, None)
    with pytest.raises(ArgumentError):
        c.norm2_cols(dA, N, K, N - 1)
    with pytest.raises(ArgumentError):
        c.norm2_cols(dA, N, 0, N)
    # pcg
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(dB, None, K, N)                      # NULL X
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(None, dA, K, N)                      # NULL B
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(dB, dA, K, N - 1)                    # ld < N
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(dB, dB, K, N)                        # X is B
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(dB, dA, K, N, nPre=3, nPost=2)       # not a symmetric preconditioner
    with pytest.raises(ArgumentError):
        H.pcg_multi_dev(dB, dA, K, N, maxiter=-1)
    # multigrid
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(None, dB, dC, 5, 1e-8, K, N)   # NULL X0
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(dA, dB, None, 5, 1e-8, K, N)   # NULL X
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(dA, dB, dC, 5, 1e-8, K, N - 1)
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(dA, dB, dA, 5, 1e-8, K, N)     # X is X0
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(dA, dB, dB, 5, 1e-8, K, N)     # X is B
    with pytest.raises(ArgumentError):
        H.multigrid_multi_dev(dA, dB, dC, 5, 1e-8, K, N, check_every=0)
    st = c.lib.aggmg_multigrid_multi_dev(c.handle, H.handle, dA.ptr, dB.ptr, K, N, 5, 1e-8, 1, 3, 3, 2.0 / 3.0, dC.ptr,
                                         np.zeros(K * 5).ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                         (ctypes.c_int * K)(), (ctypes.c_int * K)(), dA.ptr, None, None)
    assert st == _lib.ERR_ARGUMENT                           # U_exact without err_hist
    # shapes through the public functions
    with pytest.raises(DimensionMismatch):
        mg.pcg(H, np.zeros((N + 1, K)))
    with pytest.raises(DimensionMismatch):
        mg.multigrid(H, np.zeros((N, K + 1)), np.zeros((N, K)), 5, 1e-8)
    with pytest.raises(ArgumentError):
        mg.pcg(H, np.zeros((N, 0)))
    with pytest.raises(ArgumentError):
        mg.pcg(H, dB, np.zeros((N, K)))                      # device B, host X0
    # a hierarchy whose coarsest solve is the caller's
    Ho, _ = oracle.build_dg_agg_hierarchy(64, p=3, pAgg=1, nAgg=3, first=4)
    He = mg.MeshHierarchy.from_reference(Ho, ctx=c, coarse_mode=_lib.COARSE_EXTERNAL)
    Ne = He._ops[0].shape[0]
    eA, eB, eC = mg.DeviceMatrix(c, Ne, 2), mg.DeviceMatrix(c, Ne, 2), mg.DeviceMatrix(c, Ne, 2)
    with pytest.raises(ArgumentError):
        He.pcg_multi_dev(eB, eA)
    with pytest.raises(ArgumentError):
        He.multigrid_multi_dev(eA, eB, eC, 5, 1e-8)
    He.free()
