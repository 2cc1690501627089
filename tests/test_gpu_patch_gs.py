"""Multiplicative two-colour element-patch smoother on the device (aggmg_patch_gs_setup, api.ElementPatchGaussSeidel;
DESIGN.md section 20): the fused sweep kernels patch_gs_kernel / patch_gs_dict_kernel and the level path built on them.

The reference of every sweep comparison is the float64 model of tests/patch_gs_model.py: after S sweeps

    ||u_dev - u_model||_inf <= 64 eps S max(||u_model||_inf, ||u_0||_inf)

unless the model's own distance to the same sweeps in np.longdouble is larger than that on the case; then 4 x that distance
(never anything derived from the device result).  The cases where that happens are counted and may be 1 % of all at most.
Measured on an MI355X over the 4116 comparisons below: the device stays within 0.044 of the first bound everywhere, the model
within 0.037 of it of the longdouble sweeps: the exception never sets the bound.

Forward sweeps run through aggmg_smooth(_weighted)_dev.  Reverse sweeps exist as the post-smoothing of a cycle only: they run
as V(0, S) on a two-level hierarchy whose interpolation holds stored zeros, so that the coarse correction adds 0.0 and the
post-smoothing starts from the given iterate.

Operators are NON-uniform (patch_schwarz_model.random_block_tridiag): on a uniform mesh a wrong patch index is invisible.
Sizes come from the planner (aggmg_patch_gs_tile_plan): one tile's owned elements - 1, + 0, + 1, two tiles + 1, besides
2, 3, 5."""
import ctypes
import gc

import numpy as np
import pytest
import scipy.sparse as sp

import patch_gs_model as gm
import patch_schwarz_model as pm

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ALPHA = 2.0 / 3.0
WEIGHTS = [0.9, 0.35, 0.6, 0.8, 0.45, 0.7, 0.55, 0.65, 0.75, 0.5, 0.85]
SHAPES = [(1, "dense"), (2, "dense"), (2, "row"), (3, "dense"), (3, "rowcol"), (4, "row"), (4, "dense"), (5, "dense"),
          (5, "rowcol"), (8, "row")]
COUNT = {"cases": 0, "fired": 0}   # sweep comparisons, and those where the longdouble exception set the bound


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def plan(mg, m, S):
    """(elements per tile, owned elements of a launch of S sweeps, halo, most sweeps per launch)"""
    te, own, halo, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    st = mg.default_context().lib.aggmg_patch_gs_tile_plan(int(m), int(S), ctypes.byref(te), ctypes.byref(own), ctypes.byref(halo),
                                                           ctypes.byref(smax))
    assert st == 0
    return te.value, own.value, halo.value, smax.value


def sizes(mg, m, S=1):
    own = plan(mg, m, S)[1]
    assert own >= 1
    return sorted(x for x in {2, 3, 5, own - 1, own, own + 1, 2 * own + 1} if x >= 2)


def sweeps_dev(op, S, u0, b, alpha, n):
    """n forward sweeps on the device from u0 (None: the zero iterate, passed as a null pointer); alpha a number or a list"""
    c = op.ctx
    du = None if u0 is None else c.to_device(u0)
    db, dout = c.to_device(b), c.alloc(len(b))
    try:
        if np.ndim(alpha) > 0:
            w = np.ascontiguousarray(alpha[:n], dtype=np.float64)
            c.check(c.lib.aggmg_smooth_weighted_dev(c.handle, op.handle, S.handle, None if du is None else du.ptr, db.ptr,
                                                    w.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), n, dout.ptr))
        else:
            c.check(c.lib.aggmg_smooth_dev(c.handle, op.handle, S.handle, None if du is None else du.ptr, db.ptr,
                                           float(alpha), n, dout.ptr))
        return dout.download()
    finally:
        for v in (du, db, dout):
            if v is not None:
                v.free()


class Case:
    """one operator with the smoother, and the two-level hierarchy that runs its reverse sweeps"""

    def __init__(self, mg, T, ctx=None):
        self.mg, self.T, self.m, self.ne = mg, T, T.m, T.ne
        N = T.m * T.ne
        self.op = mg.DeviceOperator(T.tocsc(), ctx=ctx)
        self.S = mg.ElementPatchGaussSeidel(self.op, T.m, T.ne)
        L = sp.csc_matrix((np.zeros(N), np.arange(N), np.array([0, N])), shape=(N, 1))   # stored zeros
        assert L.nnz == N
        self.H = mg.MeshHierarchy(None, [self.op, sp.csc_matrix(np.array([[1.0]]))], [self.S], [L], ctx=self.op.ctx)

    def sweeps(self, u0, b, alpha, n, reverse=False):
        if not reverse:
            return sweeps_dev(self.op, self.S, u0, b, alpha, n)
        if np.ndim(alpha) > 0:
            # (a schedule holds MAX_SWEEP_WEIGHTS weights per half: a longer run is cycles of at most that many sweeps, one
            # after the other -- the same sweeps)
            from agglomerationmultigrid1d_amd import _lib
            u = u0
            try:
                for at in range(0, n, _lib.MAX_SWEEP_WEIGHTS):
                    w = list(alpha[at:min(n, at + _lib.MAX_SWEEP_WEIGHTS)])
                    self.H.set_sweep_weights(0, [], w)
                    u = self.mg.multigrid_v_cycle(self.H, u, b, 0, len(w))
                return u
            finally:
                self.H.clear_sweep_weights()
        return self.mg.multigrid_v_cycle(self.H, u0, b, 0, n, float(alpha))

    def free(self):
        ops, Ls = list(self.H._ops), list(self.H._Ls)
        self.H.free()
        for x in [self.S] + Ls + ops:
            x.free()


def check_sweeps(C, u0, b, alpha, n, reverse, what):
    ud = C.sweeps(u0, b, alpha, n, reverse)
    ws = list(alpha[:n]) if np.ndim(alpha) > 0 else [alpha] * n
    start = np.zeros(len(b)) if u0 is None else u0
    um = gm.gs_sweeps(C.T, start, b, ws, reverse)
    ul = gm.gs_sweeps(C.T, start, b, ws, reverse, dtype=np.longdouble)
    scale = max(np.max(np.abs(um)), np.max(np.abs(start)))
    base = 64 * EPS * n * scale
    d_model = float(np.max(np.abs(um - ul)))
    COUNT["cases"] += 1
    tol = base
    if d_model > base:
        COUNT["fired"] += 1
        tol = 4 * d_model
    d = float(np.max(np.abs(ud - um)))
    print(f"{what}: device-model {d:.3e}  model-longdouble {d_model:.3e}  bound {base:.3e}")
    assert d <= tol, f"{what}: device-model {d:.3e} > {tol:.3e} (64 eps S max|u| = {base:.3e}, model-longdouble {d_model:.3e})"
    return ud


# ---- 1. sweeps against the float64 model ------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", SHAPES)
def test_sweeps_against_model(mg, oracle, m, coupling):
    smax = plan(mg, m, 1)[3]
    assert 1 <= smax <= 8
    for S in sorted({1, 2, 3, smax, smax + 3}):
        # a run of S sweeps goes in launches of min(S, smax) sweeps (the last one the rest): sizes at the tile boundaries
        # of the first launch
        for ne in sizes(mg, m, min(S, smax)):
            T = pm.random_block_tridiag(m, ne, coupling, 1000 * S + ne)
            C = Case(mg, T)
            try:
                assert C.S.fused and C.S.kind == 3
                N = m * ne
                u0 = oracle.splitmix_normal(N, 3 + ne)
                b = oracle.splitmix_normal(N, 5 + ne)
                for reverse in (False, True):
                    for first in (u0, None):
                        for alpha in (ALPHA, 1.0, WEIGHTS):
                            a = "W" if np.ndim(alpha) else f"{alpha:.3f}"
                            check_sweeps(C, first, b, alpha, S, reverse,
                                         f"m {m} {coupling} ne {ne} S {S} {'rev' if reverse else 'fwd'} u0 {first is not None} alpha {a}")
            finally:
                C.free()


def test_model_exception_is_rare():
    """(after the sweep tests above, in file order) the longdouble exception set the bound on at most 1 % of the cases"""
    print(f"{COUNT['fired']} of {COUNT['cases']} sweep comparisons took the longdouble exception")
    assert COUNT["fired"] <= 0.01 * COUNT["cases"]


# ---- 2. bits ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", [(2, "row"), (3, "dense"), (4, "row"), (5, "rowcol"), (8, "row")])
def test_one_launch_is_single_sweeps(mg, oracle, m, coupling):
    own, smax = plan(mg, m, 1)[1], plan(mg, m, 1)[3]
    ne = 2 * own + 7
    T = pm.random_block_tridiag(m, ne, coupling, 42)
    C = Case(mg, T)
    try:
        N = m * ne
        u0, b = oracle.splitmix_normal(N, 8), oracle.splitmix_normal(N, 9)
        for reverse in (False, True):
            for S in range(2, smax + 1):
                one = C.sweeps(u0, b, WEIGHTS, S, reverse)
                assert np.array_equal(one, C.sweeps(u0, b, WEIGHTS, S, reverse))   # run to run
                u = u0
                for s in range(S):
                    u = C.sweeps(u, b, WEIGHTS[s], 1, reverse)
                assert np.array_equal(one, u), f"S = {S} in one launch != {S} launches of one sweep (reverse {reverse})"
            # chunked runs: smax + 3 sweeps are a launch of smax and one of 3
            S = smax + 3
            two = C.sweeps(C.sweeps(u0, b, WEIGHTS, smax, reverse), b, WEIGHTS[smax:], 3, reverse)
            assert np.array_equal(C.sweeps(u0, b, WEIGHTS, S, reverse), two)
        assert not np.array_equal(C.sweeps(u0, b, ALPHA, 1), C.sweeps(u0, b, ALPHA, 1, True))   # the direction arrives
    finally:
        C.free()


@pytest.fixture(scope="module")
def ctxs(mg):
    """{True: a context with the operator dictionary on, False: one with it off}"""
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    for on in (True, False):
        out[on] = mg.Context(0)
        out[on].set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def periodic(m, q, ne, coupling, seed):
    """the interior elements of a random operator of q + 2 elements, tiled with period q to ne elements (the construction of
    tests/test_gpu_patch_dictionary.py)"""
    R = pm.random_block_tridiag(m, q + 2, coupling, seed)
    idx = 1 + np.arange(ne) % q
    diag, sup = R.diag[idx], R.sup[idx]
    sub = np.zeros_like(sup)
    if coupling == "rowcol":
        sub[:] = R.sub[idx]
    else:
        sub[1:] = np.transpose(sup[:-1], (0, 2, 1))
    return pm.BlockTridiag(sub, diag, sup)


@pytest.mark.parametrize("m,coupling", SHAPES)
def test_dictionary_on_is_dictionary_off(mg, ctxs, m, coupling):
    smax = plan(mg, m, 1)[3]
    q = 3
    own = plan(mg, m, min(3, smax))[1]
    for ne in (5, own + 1, 2 * own + 1):
        T = periodic(m, q, ne, coupling, 17 * q + m)
        N = m * ne
        rng = np.random.default_rng(1000 * q + ne)
        u0, b = rng.standard_normal(N), rng.standard_normal(N)
        C = {on: Case(mg, T, ctx=ctxs[on]) for on in (True, False)}
        try:
            assert C[False].S.dictionary_classes == 0
            nc = C[True].S.dictionary_classes
            assert nc > 0 and (ne < q + 2 or q <= nc <= q + 2), (m, coupling, ne, nc)
            for reverse in (False, True):
                for n in (1, 3, smax + 3):
                    for first in (None, u0):
                        for alpha in (ALPHA, WEIGHTS):
                            u1, u0_ = (C[on].sweeps(first, b, alpha, n, reverse) for on in (True, False))
                            assert _same(u1, u0_), (m, coupling, ne, reverse, n, float(np.max(np.abs(u1 - u0_))))
                            # (a dictionary run equal to a WRONG plain run cannot pass: the model)
                            ws = list(alpha[:n]) if np.ndim(alpha) > 0 else [alpha] * n
                            start = np.zeros(N) if first is None else first
                            um = gm.gs_sweeps(T, start, b, ws, reverse)
                            assert np.max(np.abs(u1 - um)) <= 64 * EPS * n * max(np.max(np.abs(um)), np.max(np.abs(start)))
        finally:
            for on in (True, False):
                C[on].free()


@pytest.mark.parametrize("smoother", ["patchGS0", "patchGS"])
@pytest.mark.parametrize("n", [64, 3072])
def test_hierarchy_dictionary_on_is_off(mg, ctxs, n, smoother):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=(4, 2, 2))
    b = U.rhs()
    N = len(b)
    out = {}
    for on in (True, False):
        ctx = ctxs[on]
        H = build_device_hierarchy(U, ctx, smoother=smoother)
        pl = H.patch_dictionary_levels()
        if on:
            assert 0 in pl and pl[0] > 0 and H.mSmoothers[0].dictionary_classes > 0, pl
            assert sorted(pl) == ([0] if smoother == "patchGS0" else list(range(U.nlevels - 1))), pl
        else:
            assert pl == {}
        res = {}
        bd, xa, xb = ctx.to_device(b), ctx.to_device(np.zeros(N)), ctx.alloc(N)
        for _ in range(3):
            H.vcycle_dev(xa, bd, xb)
            xa, xb = xb, xa
        res["cycles"] = xa.download()
        x, it, r, _ = mg.multigrid(H, np.zeros(N), b, 100, 1e-8, exact=False)
        res["multigrid"], res["multigrid_it"], res["multigrid_res"] = x, np.array([float(it)]), np.atleast_1d(np.asarray(r, dtype=np.float64))
        x, it, r = mg.pcg(H, b, maxiter=50, tol=1e-8)
        res["pcg"], res["pcg_it"] = x, np.array([float(it)])
        assert res["multigrid_it"][0] < 100 and res["pcg_it"][0] < 50
        out[on] = res
        for v in (bd, xa, xb):
            v.free()
        sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
        H.free()
        for x in sms + ops + Ls:
            x.free()
    for key in out[True]:
        assert _same(out[True][key], out[False][key]), key


@pytest.mark.parametrize("m,coupling", SHAPES)
def test_inverse_blocks_are_the_hybrid_smoothers(mg, m, coupling):
    for ne in (2, 5, plan(mg, m, 1)[1] + 1):
        T = pm.random_block_tridiag(m, ne, coupling, 100 + ne)
        A = T.tocsc()
        op_g, op_h = mg.DeviceOperator(A), mg.DeviceOperator(A)
        G, Hy = mg.ElementPatchGaussSeidel(op_g, m, ne), mg.ElementPatchSchwarz(op_h, m, ne)
        try:
            assert G.fused and Hy.fused and G.mBlockInds.shape == (2 * m, ne - 1)
            assert np.array_equal(G.mBlockInds, Hy.mBlockInds)
            Z = G.inverse_blocks()
            assert Z.shape == (ne - 1, 2 * m, 2 * m) and np.array_equal(Z, Hy.inverse_blocks())
        finally:
            for x in (G, Hy, op_g, op_h):
                x.free()


# ---- 3. set-up refusals ---------------------------------------------------------------------------------------------------
def test_setup_refusals(mg):
    T1 = pm.random_block_tridiag(3, 1, "dense", 1)
    with pytest.raises(mg.UnsupportedError) as ei:
        mg.ElementPatchGaussSeidel(mg.DeviceOperator(T1.tocsc()), 3, 1)
    assert "one element" in str(ei.value)
    T4 = pm.random_block_tridiag(4, 6, "dense", 5)
    A = T4.tocsc().tolil()
    A[0, 23] = 0.25     # element 0 couples to element 5
    A[23, 0] = 0.25
    with pytest.raises(mg.UnsupportedError) as ei:
        mg.ElementPatchGaussSeidel(mg.DeviceOperator(A.tocsc()), 4, 6)
    assert "block tridiagonal" in str(ei.value)
    T9 = pm.random_block_tridiag(9, 4, "row", 3)
    with pytest.raises(mg.UnsupportedError) as ei:
        mg.ElementPatchGaussSeidel(mg.DeviceOperator(T9.tocsc()), 9, 4)
    assert "9 rows per element" in str(ei.value)
    # a singular patch: the operator of the hybrid smoother's test
    T = pm.random_block_tridiag(3, 6, "dense", 7)
    d = 4.0 * np.eye(3)
    T.diag[2], T.diag[3], T.sup[2], T.sub[3] = d, d, d, d   # patch {2, 3} (the third) = [[d, d], [d, d]]: its elements are regular
    with pytest.raises(mg.SingularException) as ei:
        mg.ElementPatchGaussSeidel(mg.DeviceOperator(T.tocsc()), 3, 6)
    assert "patch 3" in str(ei.value)
    # the hybrid smoother's entry point is what it was: kinds 2 / 1, and 0 for a block-Jacobi smoother
    c = mg.default_context()
    op = mg.DeviceOperator(T4.tocsc())
    for S, want in ((mg.ElementPatchSchwarz(op, 4, 6), 2), (mg.ElementPatchSchwarz(op, 4, 6, hybrid=False), 1),
                    (mg.ElementPatchSchwarz(op, 4, 6, width=3), 2), (mg.BlockJacobi(op, mg.element_patch_lists(4, 6, 1)), 0),
                    (mg.ElementPatchGaussSeidel(op, 4, 6), 3)):
        kind = ctypes.c_int(-1)
        c.check(c.lib.aggmg_smoother_patch_kind(c.handle, S.handle, ctypes.byref(kind)))
        assert kind.value == want
        S.free()


# ---- 4. hierarchy, n = 48 ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def h48(oracle):
    return oracle.build_dg_agg_hierarchy(48, p=3)


def _device_h(mg, Ho, levels, **kw):
    """the hierarchy of Ho on the device with the multiplicative patch smoother on `levels`"""
    ops = [mg.DeviceOperator(A) for A in Ho.mStiffness]
    sms = []
    for k in range(len(ops) - 1):
        if k in levels:
            m, ne = pm.level_shape(Ho, k)
            sms.append(mg.ElementPatchGaussSeidel(ops[k], m, ne))
        else:
            sms.append(Ho.mSmoothers[k])
    return mg.MeshHierarchy(Ho.mMeshes, ops, sms, Ho.mInterpolation, **kw)


@pytest.mark.parametrize("levels", [[0], [0, 1, 2]])
def test_vcycles_against_oracle(mg, oracle, h48, levels):
    Ho, b = h48
    Hm = gm.with_gs_smoothers(oracle, Ho, levels)
    Hf = _device_h(mg, Ho, levels)
    kinds = Hf.level_kinds()
    assert kinds[-1] == "coarsest" and all(kinds[k] == "fused_btd" for k in levels), kinds
    assert all(Hf.mSmoothers[k].fused for k in levels)
    A = Ho.mStiffness[0]
    x0 = oracle.splitmix_normal(len(b), 4)
    r0 = np.linalg.norm(b - A @ x0)
    for nPre, nPost in ((3, 3), (1, 1), (2, 1), (0, 2)):
        xr = oracle.multigrid_v_cycle(Hm, x0, b, nPre, nPost, ALPHA)
        xf = mg.multigrid_v_cycle(Hf, x0, b, nPre, nPost, ALPHA)
        assert np.linalg.norm(A @ (xf - xr)) <= 1e-12 * r0, (nPre, nPost)
    c = Hf.ctx
    dx0, db, d3, d1a, d1b = c.to_device(x0), c.to_device(b), c.alloc(len(b)), c.alloc(len(b)), c.alloc(len(b))
    Hf.vcycles_dev(dx0, db, d3, 3)
    Hf.vcycle_dev(dx0, db, d1a)
    Hf.vcycle_dev(d1a, db, d1b)
    Hf.vcycle_dev(d1b, db, d1a)
    assert np.array_equal(d3.download(), d1a.download())
    Hf.free()


# the CPU pins of tests/test_patch_gs_cpu.py: (cycles of multigrid, iterations of pcg) for V(1,1), V(2,2), V(3,3)
PINS = {"defaults": ((18, 10), (9, 6), (6, 5)), "weight1": ((16, 8), (8, 5), (6, 4)), "all_alpha1": ((8, 5), (4, 3), (3, 3))}


@pytest.mark.parametrize("row", sorted(PINS))
def test_solver_counts_are_the_pins(mg, oracle, h48, row):
    Ho, b = h48
    A = Ho.mStiffness[0]
    Hf = _device_h(mg, Ho, [0, 1, 2] if row == "all_alpha1" else [0])
    alpha = 1.0 if row == "all_alpha1" else ALPHA
    x0 = np.zeros(len(b))
    for n, (cyc, its) in zip((1, 2, 3), PINS[row]):
        if row == "weight1":
            Hf.set_sweep_weights(0, [1.0] * n)
        _, it, _, _ = mg.multigrid(Hf, x0, b, 100, 1e-8, exact=False, nPre=n, nPost=n, alpha=alpha)
        assert abs(it - cyc) <= 1, (row, n, it, cyc)
        x, it_p, _ = mg.pcg(Hf, b, maxiter=50, tol=1e-8, nPre=n, nPost=n, alpha=alpha)
        assert abs(it_p - its) <= 1, (row, n, it_p, its)
        assert np.linalg.norm(A @ x - b) <= 1.05e-8 * np.linalg.norm(b), (row, n)
    Hf.free()


def test_ldiv_is_symmetric_and_checkpoints_change_nothing(mg, oracle, h48):
    from agglomerationmultigrid1d_amd import _lib
    Ho, b = h48
    N = len(b)
    r1, r2 = oracle.splitmix_normal(N, 1), oracle.splitmix_normal(N, 2)
    for levels in ([0], [0, 1, 2]):
        Hf = _device_h(mg, Ho, levels)
        y1, y2 = np.zeros(N), np.zeros(N)
        mg.ldiv(y1, Hf, r1)
        mg.ldiv(y2, Hf, r2)
        a, c_ = float(y1 @ r2), float(r1 @ y2)
        assert abs(a - c_) <= 1e-10 * abs(a), (levels, a, c_)
        Hf.free()
    Hf = _device_h(mg, Ho, [0])
    c = Hf.ctx
    was = c.option(_lib.OPT_MG_CHECKPOINT, 1)
    hist = {}
    try:
        for v in (0, 1):
            c.set_option(_lib.OPT_MG_CHECKPOINT, v)
            x, n_it, r, _ = mg.multigrid(Hf, np.zeros(N), b, 100, 1e-8, exact=False)
            hist[v] = (n_it, r, x)
    finally:
        c.set_option(_lib.OPT_MG_CHECKPOINT, was)
    assert hist[0][0] == hist[1][0] and np.array_equal(np.asarray(hist[0][1]), np.asarray(hist[1][1]))
    assert np.array_equal(hist[0][2], hist[1][2])
    assert abs(hist[0][0] - 6) <= 1
    Hf.free()


# ---- 5. neighbours -----------------------------------------------------------------------------------------------------
def test_multi_column_cycle_is_the_single_cycle(mg, oracle, h48):
    Ho, b = h48
    Hf = _device_h(mg, Ho, [0])
    assert Hf.multi_info(3) == (False, 1)
    N = len(b)
    B = np.stack([b, oracle.splitmix_normal(N, 31), oracle.splitmix_normal(N, 32)], axis=1)
    X0 = oracle.splitmix_normal(3 * N, 33).reshape(N, 3)
    c = Hf.ctx
    dB, dX0, dX = mg.DeviceMatrix(c, N, 3), mg.DeviceMatrix(c, N, 3), mg.DeviceMatrix(c, N, 3)
    dB.upload(np.asfortranarray(B))
    dX0.upload(np.asfortranarray(X0))
    Hf.vcycle_multi_dev(dX0, dB, dX)
    X = dX.download()
    for j in range(3):
        assert np.array_equal(X[:, j], mg.multigrid_v_cycle(Hf, X0[:, j], B[:, j])), j
    Hf.free()


def test_dist_create_refuses(mg, oracle, h48):
    from agglomerationmultigrid1d_amd import _lib
    Ho, _ = h48
    Hl = _device_h(mg, Ho, [0], coarse_mode=_lib.COARSE_EXTERNAL)
    Hc = mg.MeshHierarchy(None, [Ho.mStiffness[-1]], [], [])
    n = Hl.nlevels
    ne = [len(mesh.mElements) for mesh in Ho.mMeshes]
    ms = [Ho.mStiffness[k].shape[0] // ne[k] for k in range(n)]
    i64 = lambda v: (ctypes.c_int64 * n)(*v)
    i32 = lambda v: (ctypes.c_int32 * n)(*v)
    zero = [0] * n
    out = ctypes.c_void_p()
    c = Hl.ctx
    st = c.lib.aggmg_dist_create(c.handle, Hl.handle, Hc.handle, 1, 0, n, i64(zero), i64(ne), i64(zero), i64(ne), i64(ne),
                                 i32(ms), i32([1] * n), ctypes.byref(out))
    assert st == _lib.ERR_UNSUPPORTED and not out.value
    with pytest.raises(mg.UnsupportedError):
        c.check(st)
    Hl.free()
    Hc.free()


def test_launch_bytes_are_the_hybrid_smoothers(mg):
    for m, coupling in ((2, "row"), (4, "dense")):
        T = pm.random_block_tridiag(m, 50, coupling, 5)
        op = mg.DeviceOperator(T.tocsc())
        G, Hy = mg.ElementPatchGaussSeidel(op, m, 50), mg.ElementPatchSchwarz(op, m, 50)
        assert mg.smoother_launch_bytes(op, G, "sweeps") == mg.smoother_launch_bytes(op, Hy, "sweeps")
        for x in (G, Hy, op):
            x.free()


def test_memory_returns(mg, oracle, h48):
    from agglomerationmultigrid1d_amd.api import device_memory
    Ho, b = h48

    def round_trip():
        op = mg.DeviceOperator(Ho.mStiffness[0])
        S = mg.ElementPatchGaussSeidel(op, 4, 48)
        assert S.fused
        held = device_memory()[1]
        mg.smooth(op, S, np.zeros(len(b)), b, ALPHA, 11)
        S.free()
        op.free()
        Hf = _device_h(mg, Ho, [0, 1, 2])
        mg.multigrid_v_cycle(Hf, np.zeros(len(b)), b)
        sms, ops, Ls = list(Hf.mSmoothers), list(Hf._ops), list(Hf._Ls)
        Hf.free()
        for x in sms + ops + Ls:
            x.free()
        return held

    round_trip()   # (the context's own work vectors grow on first use and stay)
    gc.collect()
    mg.default_context().synchronize()
    start = device_memory()
    held = round_trip()
    assert held > start[1]
    assert device_memory() == start
