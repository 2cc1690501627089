"""Operator dictionary of the fused element-patch Schwarz smoother (csrc/patch_kernels.hpp patch_sweep_dict_kernel, set-up
csrc/setup.hip setup_patch_dictionary): the smoother keeps one copy of every distinct per-element
operator record -- the element's rows of the two patch inverses, of its diagonal block and of its couplings -- and its
sweep launches index the operator by the element's class.  On a hierarchy's patch level the zero-sweep transfer launches
take the level's dictionary too.  The loads return the operator's own bits from another address and the arithmetic is
the plain kernel's, so every result must equal the run with AGGMG_OPT_OPERATOR_DICTIONARY off BIT FOR BIT (compared as
64-bit patterns): no tolerance applies to an on / off comparison anywhere.  The tests switch the option explicitly, one
context each way.

On a uniform mesh a wrong class index is invisible, so the sweep tests run on PERIODIC, strongly non-uniform operators:
the interior elements of patch_schwarz_model.random_block_tridiag(m, q + 2, ...) tiled with period q.  The record of an
element depends on its neighbours' blocks (through the two patch inverses), so the interior records repeat with period
q; the first and the last element differ by their zero inverse rows: q <= classes <= q + 2.  So that a dictionary run
equal to a WRONG plain run cannot pass, the on-result is also held to the float64 model within the bound of
tests/test_gpu_patch_schwarz.py, 64 eps S max|u|."""
import ctypes

import numpy as np
import pytest

import patch_schwarz_model as pm

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
ALPHA = 2.0 / 3.0
WEIGHTS = [0.9, 0.35, 0.6, 0.8, 0.45, 0.7, 0.55, 0.65, 0.75, 0.5, 0.85]
# (m, coupling): the SHAPES of tests/test_gpu_patch_schwarz.py
SHAPES = [(1, "dense"), (2, "dense"), (2, "row"), (3, "dense"), (3, "rowcol"), (4, "row"), (4, "dense"), (5, "dense"),
          (5, "rowcol"), (8, "row")]
RATIOS = (4, 2, 2)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


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
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def plan(ctx, m, S):
    """(elements per tile, owned elements of a launch of S sweeps, most sweeps per launch)"""
    te, own, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    assert ctx.lib.aggmg_patch_tile_plan(int(m), int(S), ctypes.byref(te), ctypes.byref(own), ctypes.byref(smax)) == 0
    return te.value, own.value, smax.value


def periodic(m, q, ne, coupling, seed):
    """the interior elements of a random operator of q + 2 elements, tiled with period q to ne elements"""
    R = pm.random_block_tridiag(m, q + 2, coupling, seed)
    idx = 1 + np.arange(ne) % q
    diag, sup = R.diag[idx], R.sup[idx]
    sub = np.zeros_like(sup)
    if coupling == "rowcol":
        sub[:] = R.sub[idx]
    else:
        sub[1:] = np.transpose(sup[:-1], (0, 2, 1))
    return pm.BlockTridiag(sub, diag, sup)


def sweeps_dev(op, S, u0, b, alpha, n):
    """n sweeps on the device from u0 (None: the zero iterate, a null pointer); alpha a number or a list"""
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


class Pair:
    """one operator with the fused smoother on the context with the dictionary and on the one without"""

    def __init__(self, mg, ctxs, T, hybrid=True):
        A = T.tocsc()
        self.op = {on: mg.DeviceOperator(A, ctx=ctxs[on]) for on in (True, False)}
        self.S = {on: mg.ElementPatchSchwarz(self.op[on], T.m, T.ne, hybrid=hybrid) for on in (True, False)}
        assert self.S[False].dictionary_classes == 0   # the option off: never a dictionary
        assert self.S[True].fused == self.S[False].fused

    def sweeps(self, u0, b, alpha, n):
        """the on-result, after it has been held to the off-result bit for bit"""
        u1 = sweeps_dev(self.op[True], self.S[True], u0, b, alpha, n)
        u0_ = sweeps_dev(self.op[False], self.S[False], u0, b, alpha, n)
        assert _same(u1, u0_), float(np.max(np.abs(u1 - u0_)))
        return u1

    def free(self):
        for on in (True, False):
            self.S[on].free()
            self.op[on].free()


# ---- 1. periodic, strongly non-uniform operators -------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3, 7])
@pytest.mark.parametrize("m,coupling", SHAPES)
def test_periodic_operators_bitwise(mg, ctxs, m, coupling, q):
    smax = plan(ctxs[True], m, 1)[2]
    # a run of S sweeps goes in launches of min(S, smax) sweeps (the last one the rest): sizes at the tile boundaries of
    # every launch the runs below make
    nes = {5}
    for s in {1, 3, min(8, smax), min(11, smax)}:
        own = plan(ctxs[True], m, s)[1]
        nes |= {own - 1, own, own + 1, 2 * own + 1}
    worst = 0.0
    for ne in sorted(x for x in nes if x >= 2):
        T = periodic(m, q, ne, coupling, 17 * q + m)
        N = m * ne
        rng = np.random.default_rng(1000 * q + ne)
        u0, b = rng.standard_normal(N), rng.standard_normal(N)
        for hybrid in (True, False):
            P = Pair(mg, ctxs, T, hybrid)
            try:
                S = P.S[True]
                assert S.fused and P.S[False].fused, (m, coupling, q, ne)
                if ne >= q + 2:
                    assert q <= S.dictionary_classes <= q + 2, (m, coupling, q, ne, S.dictionary_classes)
                else:
                    assert 1 <= S.dictionary_classes <= ne
                for n in (1, 3, 8, 11):   # 11: chunked
                    for first in (None, u0):
                        for alpha in (ALPHA, WEIGHTS):
                            u = P.sweeps(first, b, alpha, n)
                            # the on-result against the float64 model (the additive form amplifies at these weights:
                            # compared all the same, scaled by max |u|)
                            ws = list(alpha[:n]) if np.ndim(alpha) > 0 else [alpha] * n
                            um = T.sweeps(np.zeros(N) if first is None else first, b, ws, hybrid)
                            scale = max(np.max(np.abs(um)), 0.0 if first is None else np.max(np.abs(first)), 1e-300)
                            bound = 64 * EPS * n * scale
                            d = np.max(np.abs(u - um))
                            worst = max(worst, d / bound)
                            assert d <= bound, (m, coupling, q, ne, hybrid, n, d, bound)
                # aggmg_smoother_apply: one sweep of weight alpha from the zero iterate, per column
                B = rng.standard_normal((N, 2))
                y1, y0 = mg.apply_smoother(S, B, ALPHA), mg.apply_smoother(P.S[False], B, ALPHA)
                assert _same(y1, y0)
                assert np.any(y1 != 0.0)
            finally:
                P.free()
    print(f"m {m} {coupling} q {q}: sizes {sorted(nes)}, largest model distance / bound {worst:.3f}")


# ---- 2. class-count edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", [(2, "row"), (4, "row")])
def test_class_count_edges(mg, ctxs, m, coupling):
    # random, non-periodic: a class per element up to the limit, the full arrays (and no error) above it; one element is
    # the generic route; two elements are two classes (each has one zero inverse row block)
    for ne, want, fused in ((1000, 1000, True), (1500, 0, True), (1, 0, False), (2, 2, True)):
        T = pm.random_block_tridiag(m, ne, coupling, 31 + ne)
        P = Pair(mg, ctxs, T)
        try:
            assert P.S[True].fused == fused and P.S[False].fused == fused, ne
            assert P.S[True].dictionary_classes == want, (ne, P.S[True].dictionary_classes)
            if fused:
                N = m * ne
                rng = np.random.default_rng(ne)
                u0, b = rng.standard_normal(N), rng.standard_normal(N)
                for n in (1, 3, 11):
                    for first in (None, u0):
                        u = P.sweeps(first, b, WEIGHTS, n)
                        assert np.all(np.isfinite(u)) and np.any(u != 0.0)
        finally:
            P.free()


# ---- 3. hierarchies -----------------------------------------------------------------------------------------------------
_U = {}


def _uniform(n, **kw):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    key = (n, tuple(sorted(kw.items())))
    if key not in _U:
        _U[key] = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=RATIOS, **kw)
    return _U[key]


def _cpu_classes(U, k):
    """distinct per-element INPUT records (sub, diagonal, super block) of level k: every one of them is stored whole in
    the device record, so the device has at least as many classes"""
    sub, diag, sup = U.levels[k]["A"]
    ne = diag.shape[0]
    rec = np.concatenate([np.asarray(x).reshape(ne, -1) for x in (sub, diag, sup)], axis=1)
    return len(np.unique(np.ascontiguousarray(rec).view(np.uint64), axis=0))


def _cycles(mg, ctx, U, smoother, sweeps, x0, ncyc=3, weights=None, solve=True):
    """vcycle_dev x ncyc, vcycles_dev(ncyc) and the two solves -> (results, patch dictionary levels, dictionary levels)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    nPre, nPost = sweeps
    H = build_device_hierarchy(U, ctx, smoother=smoother)
    if weights:
        H.set_sweep_weights(0, *weights)
    b = U.rhs()
    N = len(b)
    start = np.zeros(N) if x0 is None else x0
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(start), ctx.alloc(N)
    for _ in range(ncyc):
        H.vcycle_dev(xa, bd, xb, nPre=nPre, nPost=nPost)
        xa, xb = xb, xa
    res = {"cycles": xa.download()}
    x0d = ctx.to_device(start)
    H.vcycles_dev(x0d, bd, xb, ncyc, nPre=nPre, nPost=nPost)
    res["loop"] = xb.download()
    if solve:
        x, it, r, _ = mg.multigrid(H, start, b, 100, 1e-8, exact=False, nPre=nPre, nPost=nPost)
        res["multigrid"], res["multigrid_it"] = x, np.array([float(it)])
        res["multigrid_res"] = np.atleast_1d(np.asarray(r, dtype=np.float64))   # (the residual history: bitwise too)
        x, it, _ = mg.fgmres(H, b, x0=start, restart=30, maxiter=100, tol=1e-8, nPre=nPre, nPost=nPost)
        res["fgmres"], res["fgmres_it"] = x, np.array([float(it)])
    out = (res, H.patch_dictionary_levels(), H.dictionary_levels())
    for v in (bd, xa, xb, x0d):
        v.free()
    sms, ops, Ls = list(H.mSmoothers), list(H._ops), list(H._Ls)
    H.free()
    for x in sms + ops + Ls:
        x.free()
    return out


def _on_off(mg, ctxs, U, smoother, sweeps=(3, 3), **kw):
    r1, pl1, dl1 = _cycles(mg, ctxs[True], U, smoother, sweeps, **kw)
    r0, pl0, dl0 = _cycles(mg, ctxs[False], U, smoother, sweeps, **kw)
    assert pl0 == {} and dl0 == {}, (pl0, dl0)
    for key in r1:
        assert _same(r1[key], r0[key]), (key, float(np.max(np.abs(r1[key] - r0[key]))))
    assert _same(r1["cycles"], r1["loop"])
    return r1, pl1, dl1


@pytest.mark.parametrize("smoother", ["patchSchwarz0", "patchSchwarz"])
@pytest.mark.parametrize("n", [64, 256, 3072, 4096, 4096 + 512])
def test_hierarchy_cycles_and_solves_bitwise(mg, ctxs, n, smoother):
    U = _uniform(n)
    patch_levels = [0] if smoother == "patchSchwarz0" else list(range(U.nlevels - 1))
    g = np.random.default_rng(n).standard_normal(len(U.rhs()))
    for sweeps in ((3, 3), (1, 2)):
        for x0 in (None, g):
            r, pl, dl = _on_off(mg, ctxs, U, smoother, sweeps, x0=x0)
            assert r["multigrid_it"][0] < 100 and r["fgmres_it"][0] < 100   # (both solves converged)
            for k in patch_levels:
                ne = U.levels[k]["ne"]
                assert k in pl and 1 <= pl[k] <= min(ne, 1024), (k, pl, ne)
                assert pl[k] >= _cpu_classes(U, k), (k, pl, _cpu_classes(U, k))
            assert sorted(pl) == patch_levels, (pl, patch_levels)
            assert 0 in dl, dl   # the level's transfer launches take the level's dictionary
    print(f"n={n} {smoother}: patch classes {pl}, level classes {dl}, CPU input classes "
          f"{ {k: _cpu_classes(U, k) for k in patch_levels} }")


def test_sweep_weight_schedule_bitwise(mg, ctxs):
    U = _uniform(4096)
    weights = ([0.5, 0.9, 1.3], [1.1, 0.7, 0.6])
    r_w, pl, _ = _on_off(mg, ctxs, U, "patchSchwarz0", weights=weights, x0=None, solve=False)
    assert 0 in pl
    r_p = _cycles(mg, ctxs[True], U, "patchSchwarz0", (3, 3), None, solve=False)[0]
    assert not _same(r_w["cycles"], r_p["cycles"]), "the schedule changed nothing: it did not reach the launch under test"


def test_mesh_with_many_roundings_bitwise(mg, ctxs):
    """a uniform mesh of an interval whose vertices round in many different ways (the mesh that overflows the fine
    level's dictionary in tests/test_gpu_pair_dictionary.py): on / off bitwise whatever the class counts are"""
    U = _uniform(160000, xin=-1.0 / 3.0, xout=1.0e9 + 0.7)
    for smoother in ("patchSchwarz0", "patchSchwarz"):
        _, pl, dl = _on_off(mg, ctxs, U, smoother, x0=None, ncyc=2, solve=False)
        print(f"{smoother}: patch classes {pl}, level classes {dl}")
        assert all(1 <= v <= 1024 for v in pl.values()) and all(1 <= v <= 1024 for v in dl.values())


# ---- 4. compulsory bytes of the sweep launch -------------------------------------------------------------------------------
@pytest.mark.parametrize("m,coupling", [(2, "row"), (4, "row"), (4, "dense"), (3, "rowcol")])
def test_launch_bytes(mg, ctxs, m, coupling):
    q, ne = 3, 50
    P = Pair(mg, ctxs, periodic(m, q, ne, coupling, 5))
    try:
        N = m * ne
        # per element: its 4 m^2 inverse-row words, its m^2 words of D_e, its couplings (scol + qrow, or sub + sup)
        rec = 8 * (4 * m * m + m * m + (2 * m if coupling != "dense" else 2 * m * m))
        nc = P.S[True].dictionary_classes
        assert q <= nc <= q + 2
        # without a dictionary: b, u, the record of every element; the new u
        assert mg.smoother_launch_bytes(P.op[False], P.S[False], "sweeps") == (16 * N + ne * rec, 8 * N)
        # with one: b, u, 2 bytes of class per element and the dictionary once; the new u
        assert mg.smoother_launch_bytes(P.op[True], P.S[True], "sweeps") == (16 * N + 2 * ne + nc * rec, 8 * N)
    finally:
        P.free()
