"""The K-column cycle on CG chain levels (AGGMG_OPT_CHAIN_MULTI, cgt_multi_kernel).

Every column of a K-column run must be BIT FOR BIT the single-column cycle of that column (compared as 64-bit patterns),
with the option on (column groups through cgt_multi_kernel) and off (column by column, the default).  The single-column
chain cycle is held to the oracle by tests/test_gpu_chain.py; one direct oracle comparison here keeps "equal to a wrong
single run" from passing.  Every K-column call runs on buffers of leading dimension N + 3 with one column more than K,
filled with NaN outside the N x K block: a read of a padding row poisons the result, a write to one is seen."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 8, 11)
KMAX = max(KS)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


@pytest.fixture(scope="module")
def ctx_on(mg):
    """a context with AGGMG_OPT_CHAIN_MULTI on"""
    from agglomerationmultigrid1d_amd import _lib
    c = mg.Context(0)
    c.set_option(_lib.OPT_CHAIN_MULTI, 1)
    return c


@pytest.fixture(scope="module")
def ctx_off(mg):
    """the default context: the option is never set on it"""
    return mg.Context(0)


@pytest.fixture(scope="module")
def ctx_on_plain(mg):
    """AGGMG_OPT_CHAIN_MULTI on, AGGMG_OPT_OPERATOR_DICTIONARY off: the variants that read the full arrays"""
    from agglomerationmultigrid1d_amd import _lib
    c = mg.Context(0)
    c.set_option(_lib.OPT_CHAIN_MULTI, 1)
    c.set_option(_lib.OPT_OPERATOR_DICTIONARY, 0)
    return c


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def plan(mg, m, S, kind, rho, kb):
    """aggmg_chain_multi_tile_plan -> (tile blocks, owned, halo left, halo right, most sweeps per launch)"""
    v = [ctypes.c_int(0) for _ in range(5)]
    st = mg.default_context().lib.aggmg_chain_multi_tile_plan(int(m), int(S), int(kind), int(rho), int(kb), *[ctypes.byref(x) for x in v])
    assert st == 0
    return tuple(x.value for x in v)


def _single(H, X0, B, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """column by column through the single-vector device cycle"""
    c = H.ctx
    N, K = B.shape
    out = np.empty((N, K))
    xo = c.alloc(N)
    for j in range(K):
        x0 = None if X0 is None else c.to_device(X0[:, j])
        H.vcycle_dev(x0, c.to_device(B[:, j]), xo, nPre, nPost, alpha)
        out[:, j] = xo.download()
    return out


def _multi(H, X0, B, nPre=3, nPost=3, alpha=2.0 / 3.0):
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
        H.vcycle_multi_dev(dX0, dB, dX, K, ld, nPre, nPost, alpha)
        out = dX.download().reshape((ld, K + 1), order="F")
    finally:
        for v in (dB, dX0, dX):
            if v is not None:
                v.free()
    assert np.isnan(out[N:, :]).all(), "rows past N were written"
    assert np.isnan(out[:, K]).all(), "the column past K was written"
    assert np.isfinite(out[:N, :K]).all(), "a padding row or column was read"
    return out[:N, :K]


def _columns(oracle, b, K, seed):
    """right-hand sides b, scaled copies of b and seeded normal vectors; non-zero staggered initial guesses"""
    N = len(b)
    B = np.column_stack([b, 2.0 * b, -0.5 * b] + [oracle.splitmix_normal(N, seed + 3 * j) for j in range(3, K)])[:, :K]
    X0 = np.column_stack([10.0 ** (-(j % 5)) * oracle.splitmix_normal(N, seed + 100 + 7 * j) for j in range(K)])
    return B, X0


def _pair(mg, Ho, ctx_on, ctx_off):
    return mg.MeshHierarchy.from_reference(Ho, ctx=ctx_on), mg.MeshHierarchy.from_reference(Ho, ctx=ctx_off)


def _check_columns(H_on, H_off, X0, B, Ks, nPre=3, nPost=3, alpha=2.0 / 3.0, fused=True, launches_per_group=None):
    """multi on H_on for every K against the single-column cycle of every column, and against H_off's columns"""
    ctx_on, ctx_off = H_on.ctx, H_off.ctx
    Kmax = B.shape[1]
    R = _single(H_on, X0, B, nPre, nPost, alpha)
    Xoff = _multi(H_off, X0, B, nPre, nPost, alpha)
    for j in range(Kmax):
        assert _same(Xoff[:, j], R[:, j]), ("off", j, float(np.max(np.abs(Xoff[:, j] - R[:, j]))))
    for K in Ks:
        assert H_on.multi_info(K, nPre, nPost) == ((True, min(K, 8)) if fused else (False, 1)), (K, H_on.multi_info(K, nPre, nPost))
        assert H_off.multi_info(K, nPre, nPost) == (False, 1)
        before = ctx_on.chain_multi_launches()
        X = _multi(H_on, None if X0 is None else X0[:, :K], B[:, :K], nPre, nPost, alpha)
        grown = ctx_on.chain_multi_launches() - before
        for j in range(K):
            assert _same(X[:, j], R[:, j]), (K, j, nPre, nPost, float(np.max(np.abs(X[:, j] - R[:, j]))))
        if not fused:
            assert grown == 0, grown
        elif launches_per_group is not None:
            assert grown == launches_per_group * -(-K // 8), (K, grown)
    assert ctx_off.chain_multi_launches() == 0


# ---- 1. the config-5 shape, bit for bit per column ------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(7))
def test_config5_columns_bitwise(mg, oracle, ctx_on, ctx_off, which):
    """CG p = 4, 2, 1 then DG p = 0: one block, a few, several tiles, and the tile boundaries of the fine descent"""
    te, own, hl, hr, smax = plan(mg, 4, 3, 1, 1, 8)
    assert te == 64 and own == te - hl - hr and own >= 8 and smax >= 3
    n = [4, 16, 130, own - 2, own - 1, own, 2 * own][which]   # n + 1 blocks: own - 1, own, own + 1, 2 own + 1
    Ho, b = oracle.build_cg_hierarchy(n, ps=(4, 2, 1), nDG=1, pDG=0)
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    try:
        assert H_on.level_kinds() == ['fused_chain'] * 3 + ['coarsest'], H_on.level_kinds()
        B, X0 = _columns(oracle, b, KMAX, n)
        _check_columns(H_on, H_off, X0, B, KS, launches_per_group=2 * 3)
        _check_columns(H_on, H_off, None, B[:, :3], (3,), launches_per_group=2 * 3)   # zero guesses
    finally:
        H_on.free()
        H_off.free()


@pytest.fixture(scope="module")
def case130(mg, oracle, ctx_on, ctx_off):
    Ho, b = oracle.build_cg_hierarchy(130, ps=(4, 2, 1), nDG=1, pDG=0)
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    B, X0 = _columns(oracle, b, KMAX, 130)
    yield dict(Ho=Ho, b=b, H_on=H_on, H_off=H_off, B=B, X0=X0)
    H_on.free()
    H_off.free()


# ---- 2. sweep counts and weights --------------------------------------------------------------------------------------------
def test_sweep_counts(mg, case130):
    d = case130
    smax = min(plan(mg, m, 1, 0, 1, 8)[4] for m in (4, 2, 1))
    assert 3 <= smax <= 8
    for nPre, nPost, alpha in ((0, 0, 2.0 / 3.0), (1, 2, 0.5), (3, 0, 2.0 / 3.0), (smax, smax, 2.0 / 3.0)):
        _check_columns(d["H_on"], d["H_off"], d["X0"][:, :4], d["B"][:, :4], (3, 4), nPre, nPost, alpha, launches_per_group=6)
    # a half-cycle of more sweeps than one launch takes: column by column, the same bits
    _check_columns(d["H_on"], d["H_off"], d["X0"][:, :3], d["B"][:, :3], (3,), smax + 1, 1, fused=False)
    _check_columns(d["H_on"], d["H_off"], d["X0"][:, :3], d["B"][:, :3], (3,), 1, smax + 1, fused=False)


def test_sweep_weight_schedules(mg, oracle, ctx_on, ctx_off):
    Ho, b = oracle.build_cg_hierarchy(130, ps=(4, 2, 1), nDG=1, pDG=0)
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    try:
        B, X0 = _columns(oracle, b, 11, 5)
        plain = _single(H_on, X0[:, :1], B[:, :1])
        sched = {0: ([0.9, 0.35, 0.6], [0.8, 0.45, 0.7]), 1: ([0.5, 0.65, 0.3], [0.55, 0.75, 0.4]), 2: ([0.7, 0.2, 0.85], [0.25, 0.95, 0.6])}
        for H in (H_on, H_off):
            for k, (pre, post) in sched.items():
                H.set_sweep_weights(k, pre, post)
        _check_columns(H_on, H_off, X0, B, (3, 11), launches_per_group=6)
        assert not _same(_single(H_on, X0[:, :1], B[:, :1]), plain)   # the schedule arrives
        for H in (H_on, H_off):
            H.clear_sweep_weights()
        # a Chebyshev schedule per chain level (estimated on each hierarchy by the same deterministic launches)
        lam_on = H_on.set_chebyshev_smoothing(levels=(0, 1, 2))
        lam_off = H_off.set_chebyshev_smoothing(levels=(0, 1, 2))
        assert lam_on == lam_off
        _check_columns(H_on, H_off, X0[:, :4], B[:, :4], (3, 4), launches_per_group=6)
    finally:
        H_on.free()
        H_off.free()


# ---- 3. non-uniform operators, with and without the dictionary ------------------------------------------------------------
@pytest.mark.parametrize("n,dictionary", [(200, True), (200, False), (1200, None)])
def test_jittered_mesh_columns_bitwise(mg, oracle, monkeypatch, ctx_on, ctx_on_plain, ctx_off, n, dictionary):
    """every interior vertex moved by a seeded +-0.3 of the element width: every block has a record of its own, so a
    wrong block or class index shows.  n = 200: a dictionary of about 200 classes per level (DICT variants), and the
    same mesh with the dictionary switched off (plain variants); n = 1200: more classes than a dictionary takes"""
    o = oracle
    uniform = o.create_uniform_mesh

    def jittered(n_, xin, xout):
        mesh = uniform(n_, xin, xout)
        d = np.random.default_rng(5).uniform(-0.3, 0.3, n_ + 1) * (xout - xin) / n_
        for v, dv in zip(mesh.mVertices[1:-1], d[1:-1]):
            v.mX += dv
        return mesh
    monkeypatch.setattr(o, "create_uniform_mesh", jittered)
    Ho, b = o.build_cg_hierarchy(n, ps=(4, 2, 1), nDG=1, pDG=0)
    H_on, H_off = _pair(mg, Ho, ctx_on_plain if dictionary is False else ctx_on, ctx_off)
    try:
        lv = H_on.dictionary_levels()
        print(f"n={n}: dictionary levels {lv}")
        if dictionary:
            assert all(k in lv and 100 <= lv[k] <= 1024 for k in range(3)), lv
        else:
            assert all(k not in lv for k in range(3)), lv
        B, X0 = _columns(o, b, 8, n)
        _check_columns(H_on, H_off, X0, B, (3, 8), launches_per_group=6)
    finally:
        H_on.free()
        H_off.free()


# ---- 4. one direct oracle comparison ------------------------------------------------------------------------------------------
def test_against_oracle(mg, oracle, case130):
    """column 2 of a K = 3 run against the oracle's cycle, at the bound tests/test_gpu_chain.py holds this shape to"""
    d = case130
    X = _multi(d["H_on"], d["X0"][:, :3], d["B"][:, :3])
    assert d["H_on"].multi_info(3) == (True, 3)
    xr = oracle.multigrid_v_cycle(d["Ho"], d["X0"][:, 2].copy(), d["B"][:, 2].copy())
    rel = np.linalg.norm(X[:, 2] - xr) / np.linalg.norm(xr)
    print(f"column 2: relative difference to the oracle {rel:.3e}")
    assert rel < 1e-8


def test_launch_bytes_count_the_operator_once(mg, case130):
    """a chain level's launch of K columns: at K = 1 the single-column figures, then a fixed number of bytes per column
    (the vectors), the operator, transfer and index arrays once"""
    H = case130["H_on"]
    for k in range(3):
        for kind in ("down", "up"):
            for x0 in (False, True):
                r1, w1 = H.multi_launch_bytes(k, kind, 1, has_x0=x0)
                assert (r1, w1) == H.launch_bytes(k, kind, has_x0=x0), (k, kind, x0)
                r2, w2 = H.multi_launch_bytes(k, kind, 2, has_x0=x0)
                rs, ws = r2 - r1, w2 - w1
                assert 0 < rs < r1 and 0 < ws <= w1 and rs % 8 == 0 and ws % 8 == 0, (k, kind, x0, r1, w1, rs, ws)
                for K in (3, 8, 11):
                    assert H.multi_launch_bytes(k, kind, K, has_x0=x0) == (r1 + (K - 1) * rs, w1 + (K - 1) * ws), (k, kind, K)


# ---- 5. other shapes ----------------------------------------------------------------------------------------------------------
def test_config1_m1_alone(mg, oracle, ctx_on, ctx_off):
    Ho, b = oracle.build_cg_hierarchy(1024, ps=(1,), nDG=1, pDG=0)   # BASELINE config 1
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    try:
        assert H_on.level_kinds() == ['fused_chain', 'coarsest']
        B, X0 = _columns(oracle, b, 11, 1)
        _check_columns(H_on, H_off, X0, B, (1, 4, 11), launches_per_group=2)
    finally:
        H_on.free()
        H_off.free()


def test_cg_coarsest_in_the_reference_numbering(mg, oracle, ctx_on, ctx_off):
    """CG p = 4, 2 over a coarsest CG p = 1 level: the last chain transfer goes through cperm"""
    Ho, b = oracle.build_cg_hierarchy(128, ps=(4, 2, 1))
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    try:
        assert H_on.level_kinds() == ['fused_chain'] * 2 + ['coarsest']
        B, X0 = _columns(oracle, b, 8, 2)
        _check_columns(H_on, H_off, X0, B, (3, 8), launches_per_group=4)
    finally:
        H_on.free()
        H_off.free()


def test_chain_levels_over_agglomerated_levels(mg, oracle, ctx_on, ctx_off):
    """the reference's full_heirarchy_test shape: the last chain level restricts into 4:1 agglomerates (owned blocks a
    multiple of the ratio), block-Jacobi levels below take the K-column block-tridiagonal launches"""
    Ho, b = oracle.build_cg_hierarchy(64, ps=(4, 2, 1), nAgg=4)
    H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    try:
        kinds = H_on.level_kinds()
        print(kinds, H_on.multi_info(4))
        assert kinds[:3] == ['fused_chain'] * 3 and kinds[-1] == 'coarsest' and len(kinds) >= 5, kinds
        assert all(k == 'fused_btd' for k in kinds[3:-1]), kinds
        assert H_on.multi_info(4)[0]
        B, X0 = _columns(oracle, b, 11, 3)
        _check_columns(H_on, H_off, X0, B, (4, 11), launches_per_group=6)
    finally:
        H_on.free()
        H_off.free()


def test_chain_detected_from_the_operators_alone(mg, oracle, ctx_on, ctx_off):
    """no element lists: the chains are recognised from the operators' patterns (their perm is the library's own)"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(256)

    def build(ctx):
        ops = [mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx) for A in U.A]
        sms = [mg.JacobiSmoother(ops[k], ctx, None, detect=True) for k in range(U.nlevels - 1)]
        Ls = [mg.DeviceOperator(L, _lib.OP_TRANSFER, ctx) for L in U.L]
        return mg.MeshHierarchy(None, ops, sms, Ls, ctx=ctx)
    H_on, H_off = build(ctx_on), build(ctx_off)
    try:
        assert H_on.level_kinds() == ['fused_chain'] * (U.nlevels - 1) + ['coarsest'], H_on.level_kinds()
        B, X0 = _columns(oracle, U.rhs(), 8, 4)
        _check_columns(H_on, H_off, X0, B, (3, 8), launches_per_group=2 * (U.nlevels - 1))
    finally:
        H_on.free()
        H_off.free()


# ---- 6. fallbacks keep (False, 1) and the bits, with the option on -----------------------------------------------------------
@pytest.mark.parametrize("shape", ["m8", "m6m3", "hybridSchwarz", "blockGS"])
def test_fallbacks_stay_column_by_column(mg, oracle, ctx_on, ctx_off, shape):
    alpha = 2.0 / 3.0
    if shape == "m8":
        Ho, b = oracle.build_cg_hierarchy(64, ps=(8, 4, 2, 1))
        H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    elif shape == "m6m3":
        Ho, b = oracle.build_cg_hierarchy(96, ps=(6, 3), nDG=2, pDG=1)
        H_on, H_off = _pair(mg, Ho, ctx_on, ctx_off)
    else:
        from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, build_device_cg_hierarchy
        U = UniformCgDgHierarchy(384)
        b = U.rhs()
        alpha = 1.0
        H_on, H_off = build_device_cg_hierarchy(U, ctx_on, smoother=shape), build_device_cg_hierarchy(U, ctx_off, smoother=shape)
    try:
        assert 'fused_chain' in H_on.level_kinds()
        B, X0 = _columns(oracle, b, 3, 6)
        _check_columns(H_on, H_off, X0, B, (3,), alpha=alpha, fused=False)
    finally:
        H_on.free()
        H_off.free()


# ---- 7. solvers ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def solver_case(mg, oracle, ctx_on):
    Ho, b = oracle.build_cg_hierarchy(256, ps=(4, 2, 1), nDG=1, pDG=0)
    H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx_on)
    N = len(b)
    u_star, _, _, _ = mg.multigrid(H, np.zeros(N), b, 200, 1e-13, exact=False)
    assert np.isfinite(u_star).all()
    noise = oracle.splitmix_normal(N, 17) * np.max(np.abs(u_star))
    yield dict(H=H, b=b, N=N, u_star=u_star, noise=noise)
    H.free()


def test_solvers_on_matrices(mg, solver_case):
    d = solver_case
    H, N, K = d["H"], d["N"], 8
    assert H.multi_info(K) == (True, 8)
    X0 = np.column_stack([d["u_star"] + 10.0 ** (-2 * j) * d["noise"] for j in range(K)])   # columns finish at different iterations
    B = np.column_stack([d["b"]] * K)
    before = H.ctx.chain_multi_launches()
    X, its, res, err = mg.multigrid(H, X0, B, 60, 1e-8, exact=False)
    assert H.ctx.chain_multi_launches() > before
    counts = []
    for j in range(K):
        xs, its0, res0, _ = mg.multigrid(H, X0[:, j].copy(), B[:, j].copy(), 60, 1e-8, exact=False)
        assert int(its[j]) == its0, (j, its[j], its0)
        assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
        assert len(res[j]) == len(res0) and np.allclose(res[j], res0, rtol=1e-10, atol=1e-13 * np.linalg.norm(d["b"])), j
        counts.append(its0)
    print("multigrid cycles per column", counts)
    assert len(set(counts)) >= 2, counts
    before = H.ctx.chain_multi_launches()
    X, its, res = mg.pcg(H, B, X0, maxiter=40, tol=1e-9)
    assert H.ctx.chain_multi_launches() > before
    counts = []
    for j in range(K):
        xs, its0, res0 = mg.pcg(H, B[:, j].copy(), X0[:, j].copy(), maxiter=40, tol=1e-9)
        assert int(its[j]) == its0, (j, its[j], its0)
        assert _same(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
        assert res[j] == res0, j
        counts.append(its0)
    print("pcg iterations per column", counts)
    assert len(set(counts)) >= 2, counts
    # ldiv on N x 3: one cycle from zero guesses
    B3 = np.column_stack([d["b"], 2.0 * d["b"], d["noise"]])
    Y = np.empty_like(B3)
    mg.ldiv(Y, H, B3)
    for j in range(3):
        y = np.empty(N)
        mg.ldiv(y, H, B3[:, j].copy())
        assert _same(Y[:, j], y), j


# ---- 8. the option is read at every call -------------------------------------------------------------------------------------
def test_option_read_per_call(mg, oracle):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    Ho, b = oracle.build_cg_hierarchy(16, ps=(4, 2, 1), nDG=1, pDG=0)
    H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
    try:
        B, X0 = _columns(oracle, b, 3, 8)
        ctx.set_option(_lib.OPT_CHAIN_MULTI, 1)
        assert H.multi_info(3) == (True, 3)
        X1 = _multi(H, X0, B)
        n1 = ctx.chain_multi_launches()
        assert n1 == 6
        ctx.set_option(_lib.OPT_CHAIN_MULTI, 0)
        assert H.multi_info(3) == (False, 1)
        X2 = _multi(H, X0, B)
        assert ctx.chain_multi_launches() == n1
        assert _same(X1, X2)
    finally:
        H.free()
