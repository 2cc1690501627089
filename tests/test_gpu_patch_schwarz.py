"""Element-patch Schwarz smoother on the device (aggmg_patch_schwarz_setup, api.ElementPatchSchwarz):
the fused sweep kernel and the level path built on it.

The reference of every comparison is the library's generic route on the same lists -- HybridSchwarzSmoother /
AdditiveSchwarzSmoother(A, element_patch_lists(m, ne)), which the fused form does not touch; the oracle's
HybridSchwarzSmoother on those lists is the second one.  The two routes apply the same inverses (held to bits below) and
differ in summation order only: after S sweeps

    ||u_fused - u_generic||_inf <= 64 eps S max(||u_generic||_inf, ||u_0||_inf, 1e-300)

unless the generic route's own distance to the float64 model (tests/patch_schwarz_model.py) is larger than that on the
case; then 4 x that distance (never anything derived from the fused result).  Measured on an MI355X over the 3203
comparisons below: the fused route stays within 0.08 of the first bound everywhere; the generic route's distance to the
model exceeds it on one case only -- the jittered DG operator after S = 1 sweep, 6.7e-14 against a bound of 4.4e-14, where
the fused route is 3.4e-15 from the generic one (max over the iterates: the first one, u_0, counts as an iterate).

Operators are NON-uniform (random, diagonally dominant block-tridiagonal ones with dense, one-row / one-column symmetric
and unsymmetric couplings, and a DG operator on a jittered mesh): on a uniform mesh all interior patches are equal and a
wrong patch or row index is invisible.  Sizes come from the planner (aggmg_patch_tile_plan): one tile's owned elements
- 1, + 0, + 1 (a last tile of one element), two tiles + 1, besides 1, 2, 3, 5."""
import ctypes
import gc

import numpy as np
import pytest

import patch_schwarz_model as pm
from fgmres_model import fgmres_model

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ALPHA = 2.0 / 3.0
WEIGHTS = [0.9, 0.35, 0.6, 0.8, 0.45, 0.7, 0.55, 0.65, 0.75, 0.5, 0.85]
# (m, coupling): every block size of the issue in every coupling form the fused kernel is instantiated for
SHAPES = [(1, "dense"), (2, "dense"), (2, "row"), (3, "dense"), (3, "rowcol"), (4, "row"), (4, "dense"), (5, "dense"),
          (5, "rowcol"), (8, "row")]


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def plan(mg, m, S):
    """(elements per tile, owned elements of a launch of S sweeps, most sweeps per launch)"""
    te, own, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    st = mg.default_context().lib.aggmg_patch_tile_plan(int(m), int(S), ctypes.byref(te), ctypes.byref(own), ctypes.byref(smax))
    assert st == 0
    return te.value, own.value, smax.value


def sizes(mg, m, S=1):
    own = plan(mg, m, S)[1]
    return sorted({1, 2, 3, 5, own - 1, own, own + 1, 2 * own + 1})


def sweeps_dev(mg, op, S, u0, b, alpha, n):
    """n sweeps on the device from u0 (None: the zero iterate, passed as a null pointer); alpha a number or a list"""
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
    """one operator with the fused smoother, the generic one on the same lists (on an operator handle of its own) and
    the float64 model"""

    def __init__(self, mg, T, hybrid=True):
        self.T, self.m, self.ne, self.hybrid = T, T.m, T.ne, hybrid
        A = T.tocsc()
        self.op_f, self.op_g = mg.DeviceOperator(A), mg.DeviceOperator(A)
        self.fused = mg.ElementPatchSchwarz(self.op_f, T.m, T.ne, hybrid=hybrid)
        lists = mg.element_patch_lists(T.m, T.ne)
        self.generic = (mg.HybridSchwarzSmoother if hybrid else mg.AdditiveSchwarzSmoother)(self.op_g, lists)

    def free(self):
        for x in (self.fused, self.generic, self.op_f, self.op_g):
            x.free()


def check_sweeps(mg, C, u0, b, alpha, n, what):
    uf = sweeps_dev(mg, C.op_f, C.fused, u0, b, alpha, n)
    ug = sweeps_dev(mg, C.op_g, C.generic, u0, b, alpha, n)
    ws = list(alpha[:n]) if np.ndim(alpha) > 0 else [alpha] * n
    um = C.T.sweeps(np.zeros(len(b)) if u0 is None else u0, b, ws, C.hybrid)
    scale = max(np.max(np.abs(ug)), 0.0 if u0 is None else np.max(np.abs(u0)), 1e-300)
    base = 64 * EPS * max(n, 1) * scale
    d_gen = np.max(np.abs(ug - um))
    tol = base if d_gen <= base else 4 * d_gen
    d = np.max(np.abs(uf - ug))
    print(f"{what}: fused-generic {d:.3e}  generic-model {d_gen:.3e}  bound {base:.3e}")
    assert d <= tol, f"{what}: fused-generic {d:.3e} > {tol:.3e} (64 eps S max|u| = {base:.3e}, generic-model {d_gen:.3e})"
    return uf


# ---- 1. set-up -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", SHAPES)
def test_setup_inverses_are_the_generic_routes(mg, m, coupling):
    for ne in sizes(mg, m):
        if ne > 300 and ne != sizes(mg, m)[-1]:
            continue   # (one large size per shape is enough for the set-up kernels)
        T = pm.random_block_tridiag(m, ne, coupling, 100 + ne)
        C = Case(mg, T)
        try:
            assert C.fused.width == 2 and C.fused.hybrid
            assert C.fused.fused == (ne >= 2), (m, coupling, ne)
            assert np.array_equal(C.fused.inverse_blocks(), C.generic.inverse_blocks()), (m, coupling, ne)
        finally:
            C.free()


def test_setup_singular_patch_and_fallbacks(mg):
    T = pm.random_block_tridiag(3, 6, "dense", 7)
    d = 4.0 * np.eye(3)
    T.diag[2], T.diag[3], T.sup[2], T.sub[3] = d, d, d, d   # patch {2, 3} (the third) = [[d, d], [d, d]]: its elements are regular
    A = T.tocsc()
    with pytest.raises(mg.SingularException) as ei:
        mg.ElementPatchSchwarz(mg.DeviceOperator(A), 3, 6)
    assert "patch 3" in str(ei.value)
    with pytest.raises(mg.SingularException):   # the generic route finds the same block
        mg.HybridSchwarzSmoother(mg.DeviceOperator(A), mg.element_patch_lists(3, 6))
    # block sizes outside the kernel's instantiations and operators that are not block tridiagonal: the generic route
    T9 = pm.random_block_tridiag(9, 4, "row", 3)
    S9 = mg.ElementPatchSchwarz(mg.DeviceOperator(T9.tocsc()), 9, 4)
    assert not S9.fused and S9.width == 2
    T4 = pm.random_block_tridiag(4, 6, "dense", 5)
    A = T4.tocsc().tolil()
    A[0, 23] = 0.25     # element 0 couples to element 5
    A[23, 0] = 0.25
    Ss = mg.ElementPatchSchwarz(mg.DeviceOperator(A.tocsc()), 4, 6)
    assert not Ss.fused
    u, b = np.arange(24.0) / 7.0, np.cos(np.arange(24.0))
    op = mg.DeviceOperator(A.tocsc())
    Sg = mg.HybridSchwarzSmoother(op, mg.element_patch_lists(4, 6))
    assert np.array_equal(sweeps_dev(mg, Ss.A, Ss, u, b, ALPHA, 2), sweeps_dev(mg, op, Sg, u, b, ALPHA, 2))
    for w in (3, 4):
        Sw = mg.ElementPatchSchwarz(mg.DeviceOperator(T4.tocsc()), 4, 6, width=w)
        assert not Sw.fused and Sw.width == w and Sw.mBlockInds.shape == (4 * w, 6 - w + 1)
    for w in (0, 1, 5):
        with pytest.raises(mg.ArgumentError):
            mg.ElementPatchSchwarz(mg.DeviceOperator(T4.tocsc()), 4, 6, width=w)


# ---- 2. sweeps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", SHAPES)
def test_sweeps_against_generic_route(mg, oracle, m, coupling):
    smax = plan(mg, m, 1)[2]
    for hybrid in (True, False):
        for S in (1, 2, 3, 8, 11):
            # the launches of a run of S sweeps take min(S, smax) sweeps (the last one the rest): sizes at the tile
            # boundaries of the first launch
            for ne in sizes(mg, m, min(S, smax)):
                T = pm.random_block_tridiag(m, ne, coupling, 1000 * S + ne)
                C = Case(mg, T, hybrid)
                try:
                    N = m * ne
                    u0 = oracle.splitmix_normal(N, 3 + ne)
                    b = oracle.splitmix_normal(N, 5 + ne)
                    # (the additive form amplifies at these weights: its sweeps are compared all the same, scaled by max |u|)
                    for first in (u0, None):
                        for alpha in (ALPHA, WEIGHTS):
                            check_sweeps(mg, C, first, b, alpha, S, f"m {m} {coupling} ne {ne} S {S} hybrid {hybrid}")
                finally:
                    C.free()


def test_sweeps_on_a_jittered_dg_operator(mg, oracle):
    from agglomerationmultigrid1d_amd import uniform
    H, b, _ = uniform.build_device_ragged_hierarchy(96, keep_host=True)
    A = H._ops[0].to_scipy().tocsc()
    m, ne = 4, 96
    op_f, op_g = mg.DeviceOperator(A), mg.DeviceOperator(A)
    Sf = mg.ElementPatchSchwarz(op_f, m, ne)
    Sg = mg.HybridSchwarzSmoother(op_g, mg.element_patch_lists(m, ne))
    assert Sf.fused
    assert np.array_equal(Sf.inverse_blocks(), Sg.inverse_blocks())
    u0 = oracle.splitmix_normal(m * ne, 1)
    for S in (1, 3, 11):
        uf = sweeps_dev(mg, op_f, Sf, u0, b, ALPHA, S)
        ug = sweeps_dev(mg, op_g, Sg, u0, b, ALPHA, S)
        um = pm.patch_sweeps(A, m, ne, u0, b, [ALPHA] * S)
        base = 64 * EPS * S * max(np.max(np.abs(ug)), np.max(np.abs(u0)))
        d_gen = np.max(np.abs(ug - um))
        tol = base if d_gen <= base else 4 * d_gen
        print(f"jittered DG S {S}: fused-generic {np.max(np.abs(uf - ug)):.3e} generic-model {d_gen:.3e} bound {base:.3e}")
        assert np.max(np.abs(uf - ug)) <= tol


# ---- 3. determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", [(2, "row"), (3, "dense"), (4, "row"), (8, "row")])
def test_launches_are_deterministic_and_tile_independent(mg, oracle, m, coupling):
    own = plan(mg, m, 1)[1]
    ne = 2 * own + 7
    T = pm.random_block_tridiag(m, ne, coupling, 42)
    C = Case(mg, T)
    N = m * ne
    u0, b = oracle.splitmix_normal(N, 8), oracle.splitmix_normal(N, 9)
    for S in (2, 3, 8, 11):
        one = sweeps_dev(mg, C.op_f, C.fused, u0, b, WEIGHTS, S)
        assert np.array_equal(one, sweeps_dev(mg, C.op_f, C.fused, u0, b, WEIGHTS, S))   # run to run
        u = u0
        for s in range(S):
            u = sweeps_dev(mg, C.op_f, C.fused, u, b, WEIGHTS[s], 1)
        assert np.array_equal(one, u), f"S = {S} in one run of launches != {S} launches of one sweep"
    # the same operator embedded at an element offset inside a longer one: the same interior bits after one sweep
    ref = sweeps_dev(mg, C.op_f, C.fused, u0, b, ALPHA, 1)
    for off in (1, 2, 3):
        pad = pm.random_block_tridiag(m, ne + off + 2, coupling, 77 + off)
        for name in ("sub", "diag", "sup"):
            getattr(pad, name)[off:off + ne] = getattr(T, name)
        pad.sub[off] = 0.0          # (T's own end blocks are zero: keep the embedded operator decoupled ...
        pad.sup[off + ne - 1] = 0.0
        pad.sup[off - 1] = 0.0      # ... from its neighbours in the residual; the PATCHES across the seam differ, so
        pad.sub[off + ne] = 0.0     # only elements 1 .. ne - 2, whose two patches lie inside, are compared)
        P = Case(mg, pad)
        ue, be = np.zeros(m * pad.ne), np.zeros(m * pad.ne)
        ue[off * m:(off + ne) * m], be[off * m:(off + ne) * m] = u0, b
        got = sweeps_dev(mg, P.op_f, P.fused, ue, be, ALPHA, 1)[off * m:(off + ne) * m]
        assert np.array_equal(got[m:-m], ref[m:-m]), f"offset {off}"
        P.free()
    C.free()


# ---- 4. apply_smoother and the eigenvalue estimate ---------------------------------------------------------------------
def _oracle_h(oracle, n, p):
    Ho, b = oracle.build_dg_agg_hierarchy(n, p=p)
    return Ho, b


def _device_h(mg, Ho, levels, generic=False, **kw):
    """the hierarchy of Ho on the device with the patch smoother on `levels` (generic: HybridSchwarzSmoother on the lists)"""
    ops = [mg.DeviceOperator(A) for A in Ho.mStiffness]
    sms = []
    for k in range(len(ops) - 1):
        if k in levels:
            m, ne = pm.level_shape(Ho, k)
            sms.append(mg.HybridSchwarzSmoother(ops[k], mg.element_patch_lists(m, ne)) if generic
                       else mg.ElementPatchSchwarz(ops[k], m, ne))
        else:
            sms.append(Ho.mSmoothers[k])
    return mg.MeshHierarchy(Ho.mMeshes, ops, sms, Ho.mInterpolation, **kw)


@pytest.fixture(scope="module")
def h48(oracle):
    return _oracle_h(oracle, 48, 3)


def test_apply_and_lambda_max_agree_with_generic_route(mg, oracle, h48):
    Ho, _ = h48
    Hf, Hg = _device_h(mg, Ho, [0, 1, 2]), _device_h(mg, Ho, [0, 1, 2], generic=True)
    for k in (0, 1):
        N = Ho.mStiffness[k].shape[0]
        B = oracle.splitmix_normal(2 * N, 21 + k).reshape(N, 2)
        yf, yg = mg.apply_smoother(Hf.mSmoothers[k], B, ALPHA), mg.apply_smoother(Hg.mSmoothers[k], B, ALPHA)
        assert np.max(np.abs(yf - yg)) <= 64 * EPS * np.max(np.abs(yg))
        m, ne = pm.level_shape(Ho, k)
        yo = pm.oracle_patch_smoother(oracle, Ho.mStiffness[k], m, ne).apply(B, ALPHA)
        assert np.max(np.abs(yf - yo)) <= 1e-12 * np.max(np.abs(yo))
        lf, lg = Hf.estimate_lambda_max(k, 40), Hg.estimate_lambda_max(k, 40)
        assert abs(lf - lg) <= 1e-10 * abs(lg), (k, lf, lg)
    Hf.free()
    Hg.free()


# ---- 5. V-cycles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(48, 3), (32, 1)])
@pytest.mark.parametrize("levels", [[0], [0, 1, 2]])
def test_vcycles_against_oracle_and_generic_route(mg, oracle, n, p, levels):
    Ho, b = _oracle_h(oracle, n, p)
    Hp = pm.with_patch_smoothers(oracle, Ho, levels)
    Hf, Hg = _device_h(mg, Ho, levels), _device_h(mg, Ho, levels, generic=True)
    kinds = Hf.level_kinds()
    assert kinds[-1] == "coarsest" and all(kinds[k] == "fused_btd" for k in levels), kinds
    assert all(Hf.mSmoothers[k].fused for k in levels)
    assert Hg.level_kinds()[0] == "generic"
    A = Ho.mStiffness[0]
    x0 = oracle.splitmix_normal(len(b), 4)
    r0 = np.linalg.norm(b - A @ x0)
    for nPre, nPost in ((3, 3), (2, 1), (0, 2)):
        xr = oracle.multigrid_v_cycle(Hp, x0, b, nPre, nPost, ALPHA)
        xf = mg.multigrid_v_cycle(Hf, x0, b, nPre, nPost, ALPHA)
        xg = mg.multigrid_v_cycle(Hg, x0, b, nPre, nPost, ALPHA)
        assert np.linalg.norm(A @ (xf - xr)) <= 1e-12 * r0, (nPre, nPost)
        assert np.linalg.norm(A @ (xf - xg)) <= 1e-12 * r0, (nPre, nPost)
    # a sweep-weight schedule on the patch level: both routes take the same weights
    for H in (Hf, Hg):
        H.set_sweep_weights(0, [0.9, 0.5, 0.7], [0.6, 0.8, 0.4])
    xf, xg = mg.multigrid_v_cycle(Hf, x0, b), mg.multigrid_v_cycle(Hg, x0, b)
    assert np.linalg.norm(A @ (xf - xg)) <= 1e-12 * r0
    for H in (Hf, Hg):
        H.clear_sweep_weights()
    c = Hf.ctx
    dx0, db, d3, d1a, d1b = c.to_device(x0), c.to_device(b), c.alloc(len(b)), c.alloc(len(b)), c.alloc(len(b))
    Hf.vcycles_dev(dx0, db, d3, 3)
    Hf.vcycle_dev(dx0, db, d1a)
    Hf.vcycle_dev(d1a, db, d1b)
    Hf.vcycle_dev(d1b, db, d1a)
    assert np.array_equal(d3.download(), d1a.download())
    Hf.free()
    Hg.free()


# ---- 6. solvers ----------------------------------------------------------------------------------------------------
def test_solvers_take_the_counts_of_the_oracle(mg, oracle, h48):
    Ho, b = h48
    Hp = pm.with_patch_smoothers(oracle, Ho, [0])
    Hf, Hbj = _device_h(mg, Ho, [0]), mg.MeshHierarchy.from_reference(Ho)
    x0 = np.zeros(len(b))
    want = pm.cycles_to_tol(oracle, Hp, b)
    assert want == 9
    _, it, res, _ = mg.multigrid(Hf, x0, b, 100, 1e-8, exact=False)
    _, it_bj, _, _ = mg.multigrid(Hbj, x0, b, 100, 1e-8, exact=False)
    assert it_bj == 72
    assert abs(it - want) <= 1 and it <= 12, (it, want)
    A = Ho.mStiffness[0]
    # flexible GMRES around V(1,1)
    xm, it_m, _ = fgmres_model(oracle, Hp, b, restart=30, maxiter=60, tol=1e-8, nPre=1, nPost=1)[:3]
    assert it_m == 9
    xf, it_f, _ = mg.fgmres(Hf, b, restart=30, maxiter=60, tol=1e-8, nPre=1, nPost=1)
    assert abs(it_f - it_m) <= 1, (it_f, it_m)
    assert np.linalg.norm(A @ xf - b) <= 1.05e-8 * np.linalg.norm(b)
    # the checked loop: the same history with and without the checkpoint launches
    from agglomerationmultigrid1d_amd import _lib
    c = Hf.ctx
    was = c.option(_lib.OPT_MG_CHECKPOINT, 1)
    hist = {}
    try:
        for v in (0, 1):
            c.set_option(_lib.OPT_MG_CHECKPOINT, v)
            x, n_it, r, _ = mg.multigrid(Hf, x0, b, 100, 1e-8, exact=False)
            hist[v] = (n_it, r, x)
    finally:
        c.set_option(_lib.OPT_MG_CHECKPOINT, was)
    assert hist[0][0] == hist[1][0] == it and hist[0][1] == hist[1][1] == res
    assert np.array_equal(hist[0][2], hist[1][2])
    Hf.free()
    Hbj.free()


# ---- 7. neighbours -------------------------------------------------------------------------------------------------
def test_multi_column_cycle_is_the_single_cycle(mg, oracle, h48):
    Ho, b = h48
    Hf = _device_h(mg, Ho, [0])
    fused, group = Hf.multi_info(3)
    assert not fused and group == 1
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


def test_memory_returns_and_other_hierarchies_keep_their_kinds(mg, oracle, h48):
    from agglomerationmultigrid1d_amd.api import device_memory
    Ho, b = h48
    H0 = mg.MeshHierarchy.from_reference(Ho)
    assert H0.level_kinds() == ["fused_btd", "fused_btd", "fused_btd", "coarsest"]
    H0.free()

    def round_trip():
        op = mg.DeviceOperator(Ho.mStiffness[0])
        S = mg.ElementPatchSchwarz(op, 4, 48)
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
