"""Sweep-weight schedules (EXTENSION: the reference damps every sweep of every level by the same alpha,
src/solvers.jl:19-50): MeshHierarchy.set_sweep_weights / aggmg_hier_set_sweep_weights give every sweep of a level its own
factor, in every launch family and through every outer solver; estimate_lambda_max and chebyshev_weights make a
Chebyshev schedule of them.

The reference for distinct weights is the V-cycle composed HERE from the oracle's public pieces (smooth_once, the
transfers, sparse_direct_solve) exactly as oracle.multigrid_v_cycle composes them, with a list of factors in place of
the scalar.  Tolerances: the residual parity of tests/test_gpu_parity.py (1e-12 of the right-hand side's norm), the
iterate at the it_tol those tests use for the same hierarchy; everything that is "the same launches" or "the same
arithmetic" is compared as 64-bit patterns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-12
W8 = [0.5, 0.9, 3.0, 0.6, 1.1, 0.7, 2.0, 0.8]


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def schedule(level, npre, npost):
    """distinct weights per sweep and per level; level 0 with (3, 3): [0.5, 0.9, 3.0] / reversed"""
    pre = [W8[(i + 3 * level) % 8] for i in range(npre)]
    post = [W8[(npost - 1 - i + 3 * level) % 8] for i in range(npost)]
    return pre, post


def ref_cycle(o, Ho, x0, b, nPre, nPost, alpha, sched, coarse_solve=None):
    """oracle.multigrid_v_cycle's composition (src/solvers.jl:19-50) with per-sweep factors: sched[k] = (pre, post) of a
    scheduled level, the others use alpha"""
    solve = coarse_solve or o.sparse_direct_solve
    n = len(Ho.mStiffness)
    u, rhs = [None] * n, [None] * n
    u[0], rhs[0] = np.asarray(x0, dtype=np.float64), np.asarray(b, dtype=np.float64)
    w = lambda k, post, i: sched[k][1 if post else 0][i] if k in sched else alpha
    for k in range(n - 1):
        if k > 0:
            u[k] = np.zeros(Ho.mStiffness[k].shape[1])
        for i in range(nPre):
            u[k] = o.smooth_once(Ho.mSmoothers[k], Ho.mStiffness[k], u[k], rhs[k], w(k, False, i))
        rhs[k + 1] = o.csc_adjoint_matvec(Ho.mInterpolation[k], rhs[k] - o.csc_matvec(Ho.mStiffness[k], u[k]))
    u[n - 1] = solve(Ho.mStiffness[n - 1], rhs[n - 1])
    for k in range(n - 2, -1, -1):
        u[k] = u[k] + o.csc_matvec(Ho.mInterpolation[k], u[k + 1])
        for i in range(nPost):
            u[k] = o.smooth_once(Ho.mSmoothers[k], Ho.mStiffness[k], u[k], rhs[k], w(k, True, i), post=True)
    return u[0]


# ---- the hierarchies: built once per module, never modified (schedules are set and cleared by every test) ------------
_CACHE = {}


def case(o, mg, name):
    """-> (Ho, b, H, it_tol, alpha): oracle hierarchy, right-hand side, device hierarchy, the iterate tolerance the parity
    tests use for it (None: residual only) and the damping of its unscheduled levels"""
    if name in _CACHE:
        return _CACHE[name]
    from agglomerationmultigrid1d_amd import _lib
    alpha, it_tol = 2.0 / 3.0, 1e-9
    if name.startswith("dg"):                     # config 3 shape: DG p = 3, agglomerated 4:1, 2:1, 2:1; block Jacobi
        Ho, b = o.build_dg_agg_hierarchy(int(name[2:]), p=3, pAgg=1, nAgg=3, first=4)
        H = mg.MeshHierarchy.from_reference(Ho)
        assert all(H.structured_levels())
    elif name.startswith("gs"):                   # the same operators, red-black block Gauss-Seidel on every level
        Ho, b = o.build_dg_agg_hierarchy(int(name[2:]), p=3, pAgg=1, nAgg=3, first=4)
        Ho.mSmoothers = [o.BlockGaussSeidelRB(S.mBlocks, S.mBlockInds) for S in Ho.mSmoothers]
        H = mg.MeshHierarchy.from_reference(Ho)
        assert all(H.structured_levels())
        it_tol = None                             # (tests/test_gpu_blockgs.py holds these cycles to the residual alone)
    elif name.startswith("cg"):                   # config 5 shape: CG p = 4, 2, 1 point Jacobi, then DG p = 0
        Ho, b = o.build_cg_hierarchy(int(name[2:]), ps=(4, 2, 1), nDG=1, pDG=0)
        H = mg.MeshHierarchy.from_reference(Ho)
        assert H.level_kinds() == ['fused_chain'] * 3 + ['coarsest']
        it_tol = 1e-8
    elif name.startswith("schwarz"):              # element (hybrid) Schwarz on every CG level, alpha = 1
        Ho, b = o.build_cg_hierarchy(int(name[7:]), ps=(4, 2, 1), nDG=1, pDG=0)
        for k in range(3):
            Ho.mSmoothers[k] = o.cg_smoother(Ho.mMeshes[k], Ho.mStiffness[k], "hybridSchwarz")
        H = mg.MeshHierarchy.from_reference(Ho)
        assert H.level_kinds() == ['fused_chain'] * 3 + ['coarsest']
        alpha, it_tol = 1.0, 1e-8
    elif name.startswith("generic"):              # chain detection off: generic CSR levels, csr_band_kernel on the p = 1 one
        Ho, b = o.build_cg_hierarchy(int(name[7:]), ps=(4, 2, 1), nDG=1, pDG=0)
        ctx = mg.default_context()
        ctx.set_option(_lib.OPT_DETECT_CHAIN, 0)
        try:
            H = mg.MeshHierarchy(None, Ho.mStiffness, Ho.mSmoothers, Ho.mInterpolation)
        finally:
            ctx.set_option(_lib.OPT_DETECT_CHAIN, 1)
        assert H.level_kinds() == ['generic'] * 3 + ['coarsest']
        it_tol = 1e-8
    else:
        raise KeyError(name)
    _CACHE[name] = (Ho, b, H, it_tol, alpha)
    return _CACHE[name]


def set_all(H, npre, npost, levels=None):
    sched = {}
    for k in (range(H.nlevels - 1) if levels is None else levels):
        sched[k] = schedule(k, npre, npost)
        H.set_sweep_weights(k, *sched[k])
    return sched


def cycles(mg, H, x0, b, n, nPre, nPost, alpha):
    x = x0
    for _ in range(n):
        x = mg.multigrid_v_cycle(H, x, b, nPre=nPre, nPost=nPost, alpha=alpha)
    return x


ALL_CASES = ["dg48", "dg256", "dg3072", "cg48", "cg256", "gs48", "gs256", "schwarz64", "generic64"]


# ---- 1. a constant schedule is the scalar ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_constant_schedule_is_the_scalar(oracle, mg, name):
    o = oracle
    Ho, b, H, _, _ = case(o, mg, name)
    a = 0.61
    x0 = o.splitmix_normal(len(b), 3)
    plain = cycles(mg, H, x0, b, 2, 3, 3, a)
    try:
        for k in range(H.nlevels - 1):
            H.set_sweep_weights(k, [a, a, a])
            pre, post = H.sweep_weights(k)
            assert pre.tolist() == [a, a, a] and post.tolist() == [a, a, a]
        # (the entry point's alpha is ignored on scheduled levels)
        assert same_bits(cycles(mg, H, x0, b, 2, 3, 3, 0.123), plain)
    finally:
        H.clear_sweep_weights()
    assert all(H.sweep_weights(k) is None for k in range(H.nlevels - 1))
    assert same_bits(cycles(mg, H, x0, b, 2, 3, 3, a), plain)


def test_constant_schedule_is_the_scalar_ragged(mg):
    """agglomerates of different sizes (parent / first-child maps, atomically restricted cut agglomerates)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_ragged_hierarchy
    H, b, info = build_device_ragged_hierarchy(300, generic=True)
    a = 0.61
    x0 = np.zeros(len(b))
    plain = cycles(mg, H, x0, b, 2, 3, 3, a)
    for k in range(H.nlevels - 1):
        H.set_sweep_weights(k, [a, a, a])
    assert same_bits(cycles(mg, H, x0, b, 2, 3, 3, 0.123), plain)
    H.clear_sweep_weights()
    assert same_bits(cycles(mg, H, x0, b, 2, 3, 3, a), plain)
    # distinct weights: the fused launches against the generic kernels on the same operators (the unfused composition)
    Hg = info["generic"]
    for HH in (H, Hg):
        set_all(HH, 3, 3)
    xf, xg = cycles(mg, H, x0, b, 2, 3, 3, a), cycles(mg, Hg, x0, b, 2, 3, 3, a)
    assert not same_bits(xf, plain)
    r = mg.residual(H._ops[0], xf, b) - mg.residual(H._ops[0], xg, b)
    assert np.linalg.norm(r) <= TOL * np.linalg.norm(b)
    assert rel(xf, xg) < 1e-9


# ---- 2. distinct weights against the oracle-composed cycle ----------------------------------------------------------
# (6, 7): more sweeps than one launch takes -- the schedule crosses a launch-chunk boundary.  The several-tile size runs
# V(3,3) and V(2,4); its chunked launches are those of n = 256.
SWEEPS = [(name, s) for name in ALL_CASES for s in ((3, 3), (2, 4), (6, 7)) if not (name == "dg3072" and s == (6, 7))]


@pytest.mark.parametrize("name,sweeps", SWEEPS, ids=lambda v: v if isinstance(v, str) else "V%d%d" % v)
def test_distinct_weights_match_the_composed_cycle(oracle, mg, name, sweeps):
    o = oracle
    Ho, b, H, it_tol, alpha = case(o, mg, name)
    nPre, nPost = sweeps
    A = Ho.mStiffness[0]
    x0 = np.zeros(len(b))
    try:
        # every level but the last smoothed one is scheduled: that one keeps the entry point's alpha
        sched = set_all(H, nPre, nPost, levels=range(H.nlevels - 2))
        xr, xg = x0, x0
        for ncyc in (1, 2, 3):
            xr = ref_cycle(o, Ho, xr, b, nPre, nPost, alpha, sched)
            xg = mg.multigrid_v_cycle(H, xg, b, nPre=nPre, nPost=nPost, alpha=alpha)
            if ncyc == 2:
                continue
            scale = np.linalg.norm(b) if it_tol is not None else \
                max(np.linalg.norm(b), np.linalg.norm(A @ xr))      # (Gauss-Seidel: tests/test_gpu_blockgs.py's scale)
            dres, drel = np.linalg.norm(A @ (xg - xr)) / scale, rel(xg, xr)
            print(f"{name} V({nPre},{nPost}) after {ncyc}: residual diff {dres:.3e} of the scale, iterate diff {drel:.3e}")
            assert dres <= TOL, (name, sweeps, ncyc)
            if it_tol is not None:
                assert drel < it_tol, (name, sweeps, ncyc)
    finally:
        H.clear_sweep_weights()
    assert rel(cycles(mg, H, x0, b, 3, nPre, nPost, alpha), xg) > 1e-6     # (... and it changed the result)


# ---- 3. one launch against chained launches -------------------------------------------------------------------------
@pytest.mark.parametrize("name,level", [("dg256", 0), ("dg48", 1), ("cg256", 0), ("gs256", 0), ("schwarz64", 0),
                                        ("generic64", 2), ("generic64", 0)])
def test_weighted_smooth_is_the_chained_sweeps(oracle, mg, name, level):
    """smooth(alpha = [w0 .. w3]) -- one fused launch on the structured levels, one csr_band_kernel launch on the banded
    p = 1 operator -- against four single-sweep calls; 1e-12 in the relative 2-norm, the project's TOL for smoothed
    iterates (the block-tridiagonal kernels sum a row's products in another order with their neighbours in LDS)"""
    o = oracle
    Ho, b, H, _, _ = case(o, mg, name)
    A, S = H._ops[level], H.mSmoothers[level]
    N = Ho.mStiffness[level].shape[0]
    u0, rhs = o.splitmix_normal(N, 11), o.splitmix_normal(N, 12)
    w = [0.5, 0.9, 3.0, 0.6]
    one = mg.smooth(A, S, u0, rhs, alpha=w)
    chained = u0
    for wi in w:
        chained = mg.smooth(A, S, chained, rhs, alpha=wi, nsweeps=1)
    assert rel(one, chained) <= TOL
    # ... and against the oracle's sweeps
    uo = u0
    for wi in w:
        uo = o.smooth_once(Ho.mSmoothers[level], Ho.mStiffness[level], uo, rhs, wi)
    assert rel(one, uo) <= TOL
    # equal weights: the scalar call's bits; more sweeps than one launch takes: chunked, each chunk with its slice
    assert same_bits(mg.smooth(A, S, u0, rhs, alpha=[0.7] * 4), mg.smooth(A, S, u0, rhs, alpha=0.7, nsweeps=4))
    w11 = [0.5, 0.9, 1.4, 0.6, 1.1, 0.7, 1.3, 0.8, 0.55, 0.95, 1.2]
    long = mg.smooth(A, S, u0, rhs, alpha=w11)
    uo = u0
    for wi in w11:
        uo = o.smooth_once(Ho.mSmoothers[level], Ho.mStiffness[level], uo, rhs, wi)
    assert rel(long, uo) <= TOL
    with pytest.raises(mg.ArgumentError):
        mg.smooth(A, S, u0, rhs, alpha=[0.5, float("nan")])


# ---- 4. launch families ---------------------------------------------------------------------------------------------
def test_launch_families_give_the_same_bits(oracle, mg):
    """AGGMG_OPT_PAIR_LEVELS, _OPERATOR_DICTIONARY, _SYMMETRIC_RESIDUAL "change no bit of any result": nor of a weighted
    one, with different weights on the two levels of a paired launch"""
    from agglomerationmultigrid1d_amd import _lib
    o = oracle
    Ho, b = o.build_dg_agg_hierarchy(256, p=3, pAgg=1, nAgg=3, first=4)
    ctx = mg.default_context()
    x0 = o.splitmix_normal(len(b), 5)
    opts = (_lib.OPT_PAIR_LEVELS, _lib.OPT_OPERATOR_DICTIONARY, _lib.OPT_SYMMETRIC_RESIDUAL)

    def run(values):
        for opt, v in zip(opts, values):
            ctx.set_option(opt, v)
        try:     # (the dictionary and the symmetric form are built with the hierarchy, the pairing is decided per launch)
            H = mg.MeshHierarchy.from_reference(Ho)
            set_all(H, 3, 3)
            x = cycles(mg, H, x0, b, 2, 3, 3, 2.0 / 3.0)
            dx, dy = ctx.to_device(x0), ctx.alloc(len(b))
            H.vcycles_dev(dx, ctx.to_device(b), dy, 3)
            return (x, dy.download(), H.paired_levels(), H.paired_levels(direction="up"), H.dictionary_levels(),
                    H.sym_residual_levels())
        finally:
            for opt in opts:
                ctx.set_option(opt, 1)

    base = run((1, 1, 1))
    assert base[2] == [1] and base[3] == [1] and 0 in base[4] and base[5], "the default launches are not the ones under test"
    for values in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)):
        got = run(values)
        if values[0] == 0:
            assert got[2] == [] and got[3] == []
        if values[1] == 0:
            assert got[4] == {}
        if values[2] == 0:
            assert got[5] == []
        assert same_bits(got[0], base[0]) and same_bits(got[1], base[1]), values


# ---- 5. merged launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dg48", "dg256", "dg3072", "cg256"])
@pytest.mark.parametrize("sweeps", [(3, 3), (2, 4)], ids=lambda s: "V%d%d" % s)
def test_merged_launches(oracle, mg, name, sweeps):
    """vcycles_dev runs one cycle's post-smoothing and the next one's pre-smoothing in ONE launch (post ++ pre);
    multigrid_dev(check_every = 1) forms its residual norms inside those launches (the checkpoint kernels)"""
    o = oracle
    Ho, b, H, _, alpha = case(o, mg, name)
    nPre, nPost = sweeps
    ctx = H.ctx
    nb = np.linalg.norm(b)
    A = Ho.mStiffness[0]
    x0 = o.splitmix_normal(len(b), 6)
    try:
        set_all(H, nPre, nPost)
        db, dx, dy = ctx.to_device(b), ctx.to_device(x0), ctx.alloc(len(b))
        H.vcycles_dev(dx, db, dy, 3, nPre=nPre, nPost=nPost, alpha=alpha)
        merged = dy.download()
        d1, d2 = ctx.alloc(len(b)), ctx.alloc(len(b))
        H.vcycle_dev(dx, db, d1, nPre=nPre, nPost=nPost, alpha=alpha)
        H.vcycle_dev(d1, db, d2, nPre=nPre, nPost=nPost, alpha=alpha)
        H.vcycle_dev(d2, db, d1, nPre=nPre, nPost=nPost, alpha=alpha)
        assert same_bits(merged, d1.download())
        # the checkpointed loop: histories against explicit residual norms of the unchecked loop's iterates, held to what
        # tests/test_gpu_solvers.py holds the scalar case to (rtol 1e-10, atol 1e-13 ||b||)
        K = 5
        xc, itc, resc, _ = mg.multigrid(H, x0, b, K, 0.0, exact=False, check_every=1, nPre=nPre, nPost=nPost, alpha=alpha)
        assert itc == K and len(resc) == K
        explicit = []
        for k in range(1, K + 1):
            xk, itk, resk, _ = mg.multigrid(H, x0, b, k, 0.0, exact=False, check_every=K + 1, nPre=nPre, nPost=nPost, alpha=alpha)
            assert itk == k and len(resk) == 1
            explicit.append(np.linalg.norm(A @ xk - b))
        assert np.allclose(resc, explicit, rtol=1e-10, atol=1e-13 * nb)
        assert same_bits(xc, xk)     # (the iterates: the same arithmetic, as tests/test_gpu_solvers.py holds the scalar case)
    finally:
        H.clear_sweep_weights()


# ---- 6. K columns ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 9])
@pytest.mark.parametrize("name", ["dg48", "dg256"])
def test_every_column_is_the_single_vector_cycle(oracle, mg, name, K):
    o = oracle
    Ho, b, H, _, alpha = case(o, mg, name)
    ctx = H.ctx
    N = len(b)
    fused, group = H.multi_info(K)
    if name == "dg256":
        assert fused and group == min(K, 8), "the K-column kernel is not the one under test"
    B = np.column_stack([o.splitmix_normal(N, 20 + j) for j in range(K)])
    X0 = np.column_stack([o.splitmix_normal(N, 40 + j) for j in range(K)])
    try:
        set_all(H, 3, 3)
        dB, dX0, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
        dB.upload(B)
        dX0.upload(X0)
        H.vcycle_multi_dev(dX0, dB, dX, nPre=3, nPost=3, alpha=alpha)
        X = dX.download()
        for j in range(K):
            assert same_bits(X[:, j], mg.multigrid_v_cycle(H, X0[:, j], B[:, j], nPre=3, nPost=3, alpha=alpha)), j
        with pytest.raises(mg.ArgumentError):
            H.vcycle_multi_dev(dX0, dB, dX, nPre=2, nPost=3, alpha=alpha)
    finally:
        H.clear_sweep_weights()


# ---- 7. the estimator -----------------------------------------------------------------------------------------------
EST_TOL = 1.8e-14


def numpy_power_iteration(o, A, S, v0, iters):
    v, lam = np.array(v0, dtype=np.float64), 0.0
    for _ in range(iters):
        w = o.smooth_once(S, A, np.zeros(len(v)), o.csc_matvec(A, v), 1.0)     # S^-1 (A v)
        nw = np.linalg.norm(w)
        lam = nw / np.linalg.norm(v)
        v = w / nw
    return lam


@pytest.mark.parametrize("name", ["dg48", "dg256", "cg48", "cg256"])
def test_estimate_lambda_max(oracle, mg, name):
    """estimate_lambda_max against the same 40 steps of power iteration in NumPy on the oracle's operator and smoother.
    Tolerance EST_TOL = 1.8e-14 relative, MEASURED rather than guessed: the NumPy iteration was run on the twelve (shape,
    level) cases of this test with its two norms summed in three different orders (np.dot, math.fsum, a reversed running
    sum); the estimates differed by at most 1.8e-15 relative (config 3 shape, n = 48, level 2; 1.1e-16 .. 4.5e-16
    elsewhere), and ten times that is the bound.  At n = 48 also against the dense largest eigenvalue of S^-1 A: the
    estimate lies in [0.97, 1 + 1e-12] of it (the CPU iteration gave 0.989 .. 0.995 on all three levels of both shapes)."""
    o = oracle
    Ho, b, H, _, _ = case(o, mg, name)
    for level in range(3):
        A, S = Ho.mStiffness[level], Ho.mSmoothers[level]
        N = A.shape[0]
        v0 = o.splitmix_normal(N, 7 + level)
        lam = H.estimate_lambda_max(level, iters=40, v0=v0)
        ref = numpy_power_iteration(o, A, S, v0, 40)
        print(f"{name} level {level}: device {lam:.16f} numpy {ref:.16f} relative difference {abs(lam - ref) / ref:.3e}")
        assert abs(lam - ref) <= EST_TOL * ref, (name, level)
        # the start vector from the device, and the fixed seeded one: reproducible, near the same eigenvalue
        assert H.estimate_lambda_max(level, iters=40, v0=H.ctx.to_device(v0)) == lam
        seeded = H.estimate_lambda_max(level)
        assert seeded == H.estimate_lambda_max(level, iters=40, v0=None) and 0.9 * ref < seeded < 1.1 * ref
        if name.endswith("48"):
            Ad = A.toarray()
            SA = np.column_stack([o.smooth_once(S, A, np.zeros(N), Ad[:, j], 1.0) for j in range(N)])
            top = np.max(np.abs(np.linalg.eigvals(SA)))
            assert 0.97 * top <= lam <= (1.0 + 1e-12) * top, (name, level, lam, top)
    with pytest.raises(mg.ArgumentError):
        H.estimate_lambda_max(H.nlevels - 1)
    with pytest.raises(mg.ArgumentError):
        H.estimate_lambda_max(0, iters=0)


# ---- 8. it converges faster -----------------------------------------------------------------------------------------
def test_chebyshev_schedule_halves_the_cycle_count(oracle, mg):
    o = oracle
    Ho, b = o.build_dg_agg_hierarchy(256, p=3, pAgg=1, nAgg=3, first=4)
    H = mg.MeshHierarchy.from_reference(Ho)
    A = Ho.mStiffness[0]
    nb = np.linalg.norm(b)
    x0 = np.zeros(len(b))
    _, plain_cycles, _, _ = mg.multigrid(H, x0, b, 200, 1e-8, exact=False)
    _, plain_pcg, _ = mg.pcg(H, b, maxiter=50, tol=1e-8)
    lams = H.set_chebyshev_smoothing()
    assert list(lams) == [0] and 1.9 < lams[0] < 2.0
    pre, post = H.sweep_weights(0)
    assert same_bits(pre, mg.chebyshev_weights(lams[0])) and same_bits(post, pre[::-1])
    assert H.sweep_weights(1) is None
    sched = {0: (list(pre), list(post))}
    cyc = lambda x, r: ref_cycle(o, Ho, x, r, 3, 3, 2.0 / 3.0, sched)
    # the composed loop (oracle.multigrid's test, src/solvers.jl:124-131)
    x, ref_cycles = x0, 0
    while ref_cycles < 200:
        x = cyc(x, b)
        ref_cycles += 1
        if np.linalg.norm(A @ x - b) < 1e-8 * nb:
            break
    xg, got_cycles, res, _ = mg.multigrid(H, x0, b, 200, 1e-8, exact=False)
    print(f"cycles to 1e-8: unscheduled {plain_cycles}, Chebyshev schedule {got_cycles}, composed reference {ref_cycles}")
    assert abs(got_cycles - ref_cycles) <= 1
    assert got_cycles < plain_cycles
    assert np.linalg.norm(A @ xg - b) < 1e-8 * nb
    # conjugate gradients around the composed cycle: oracle.pcg_ldiv's recurrence
    zero = np.zeros(len(b))
    xp = zero.copy()
    r = b - o.csc_matvec(A, xp)
    z = cyc(zero, r)
    p, rz, ref_pcg = z.copy(), float(r @ z), 0
    for _ in range(50):
        q = -o.csc_matvec(A, p)
        a = rz / (-(float(p @ q)))
        xp, r = xp + a * p, r + a * q
        ref_pcg += 1
        if np.linalg.norm(r) < 1e-8 * nb:
            break
        z = cyc(zero, r)
        rz_new = float(r @ z)
        p, rz = z + (rz_new / rz) * p, rz_new
    xq, got_pcg, _ = mg.pcg(H, b, maxiter=50, tol=1e-8)
    print(f"pcg iterations to 1e-8: unscheduled {plain_pcg}, Chebyshev schedule {got_pcg}, composed reference {ref_pcg}")
    assert abs(got_pcg - ref_pcg) <= 1
    assert np.linalg.norm(A @ xq - b) < 1e-7 * nb


# ---- 9. errors ------------------------------------------------------------------------------------------------------
def test_errors_leave_the_hierarchy_usable(oracle, mg):
    from agglomerationmultigrid1d_amd import _lib
    o = oracle
    Ho, b, H, _, alpha = case(o, mg, "dg48")
    x0 = np.zeros(len(b))
    plain = cycles(mg, H, x0, b, 1, 3, 3, alpha)
    ctx = H.ctx
    try:
        H.set_sweep_weights(0, [0.5, 0.9, 3.0])
        good = cycles(mg, H, x0, b, 1, 3, 3, alpha)
        db, dx, dy = ctx.to_device(b), ctx.to_device(x0), ctx.alloc(len(b))
        for nPre, nPost in ((2, 3), (3, 2), (4, 4), (0, 3)):
            with pytest.raises(mg.ArgumentError):
                mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost)
            with pytest.raises(mg.ArgumentError):
                H.vcycles_dev(dx, db, dy, 3, nPre=nPre, nPost=nPost)
            with pytest.raises(mg.ArgumentError):
                mg.multigrid(H, x0, b, 5, 1e-8, exact=False, nPre=nPre, nPost=nPost)
            with pytest.raises(mg.ArgumentError):
                mg.pcg(H, b, maxiter=5, nPre=nPre, nPost=nPost)
        with pytest.raises(mg.ArgumentError):
            H.set_sweep_weights(0, [0.5] * (_lib.MAX_SWEEP_WEIGHTS + 1))
        with pytest.raises(mg.ArgumentError):
            H.set_sweep_weights(0, [0.5] * 3, [0.5] * (_lib.MAX_SWEEP_WEIGHTS + 1))
        for bad in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(mg.ArgumentError):
                H.set_sweep_weights(0, [0.5, bad, 0.7])
            with pytest.raises(mg.ArgumentError):
                H.set_sweep_weights(0, [0.5, 0.6, 0.7], [0.5, 0.6, bad])
        for level in (-1, H.nlevels - 1, H.nlevels):       # out of range; the coarsest level is solved, not smoothed
            with pytest.raises(mg.ArgumentError):
                H.set_sweep_weights(level, [0.5, 0.9, 3.0])
            with pytest.raises(mg.ArgumentError):
                H.sweep_weights(level)
        # every refusal left the schedule and the hierarchy as they were
        pre, post = H.sweep_weights(0)
        assert pre.tolist() == [0.5, 0.9, 3.0] and post.tolist() == [3.0, 0.9, 0.5]
        assert same_bits(cycles(mg, H, x0, b, 1, 3, 3, alpha), good)
        # the full length is accepted
        H.set_sweep_weights(1, [0.5] * _lib.MAX_SWEEP_WEIGHTS)
        assert len(H.sweep_weights(1)[0]) == _lib.MAX_SWEEP_WEIGHTS
        H.clear_sweep_weights(1)
        assert H.sweep_weights(1) is None and H.sweep_weights(0) is not None
    finally:
        H.clear_sweep_weights()
    assert same_bits(cycles(mg, H, x0, b, 1, 3, 3, alpha), plain)


# ---- the partitioned cycle refuses a schedule -----------------------------------------------------------------------
def _refusal_worker(q):
    """two ranks as threads of this (fresh) process sharing the GPU; -> [(refused, same bits afterwards, scale)] per rank"""
    import os
    import sys
    import threading
    import traceback
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [root, os.path.join(root, "oracle")]
    import torch
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    torch.cuda.init()          # (once, before the rank threads use it)
    world, n, p, ratios = 2, 2 ** 12, 3, (4, 2, 2)
    group = D.ThreadGroup(world)
    out, errs = [None] * world, []

    def rank_fn(rank):
        comm = D.ThreadComm(group, rank)
        ctx = mg.Context(0)
        layout = D.RankLayout(n, ratios, [p + 1, 2, 2, 2], world, rank)
        engine, U = D.build_local_uniform(n, p, 1, ratios, layout, ctx, comm)
        dv = D.NativeDistributedVCycle(engine, layout, comm, collectives="torch")
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        nloc = layout.local_dofs(0)

        def cycle():
            x, y = engine.new(nloc), engine.new(nloc)
            dv.vcycle(x, b, y)
            torch.cuda.synchronize()
            return y.cpu().numpy()[layout.owned_slice(0)]

        before = cycle()
        engine.H.set_sweep_weights(0, [0.5, 0.9, 3.0])
        refused = False
        try:
            cycle()
        except mg.UnsupportedError:
            refused = True
        comm.barrier()
        engine.H.clear_sweep_weights()
        after = cycle()
        comm.barrier()
        dv.free()
        return refused, same_bits(before, after), float(np.max(np.abs(before)))

    def one(r):
        try:
            out[r] = rank_fn(r)
        except BaseException:
            errs.append((r, traceback.format_exc()))
            group.barrier.abort()

    ts = [threading.Thread(target=one, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(300)
    q.put((out, errs))


def test_partitioned_cycle_refuses_a_scheduled_hierarchy():
    """aggmg_dist_vcycle_dev does not honour sweep weights, so it must not ignore them either: a schedule on
    a rank's hierarchy is AGGMG_ERR_UNSUPPORTED before anything is enqueued or exchanged, and after clear_sweep_weights the
    cycle gives the bits it gave before.  Two thread ranks in a process of their own, as the other partitioned tests of the
    single-GPU test files run theirs."""
    import torch.multiprocessing as tmp
    sp = tmp.get_context("spawn")
    q = sp.Queue()
    pr = sp.Process(target=_refusal_worker, args=(q,))
    pr.start()
    out, errs = q.get(timeout=300)
    pr.join(300)
    assert pr.exitcode == 0
    assert not errs, errs[0][1]
    for refused, same, scale in out:
        assert refused and same and scale > 0.0
