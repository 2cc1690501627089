"""Every block form a tiled kernel family is instantiated for still launches, and the first form off a list takes the
route beside it (csrc/forms.hpp: btd_form, patch_form, multi_form and the column groups of col_group).

The other GPU tests reach the forms their hierarchies happen to produce; this file walks the lists.  Operators are
NON-uniform (patch_schwarz_model.random_block_tridiag: coupling "row" is stored compressed for m >= 2, "dense" dense), so a
launch of the wrong instantiation or a wrong index shows.  Sizes: 3 elements, and one tile's owned elements + 1 (a second
tile of one element) from the family's tile plan.

Tolerance of the two comparisons against a reference (tests/test_gpu_patch_schwarz.py's rule): after S sweeps

    ||u_dev - u_ref||_inf <= 64 eps S max(||u_ref||_inf, ||u_0||_inf, 1e-300)

unless the reference's own distance to the float64 model is larger than that on the case; then 4 x that distance (never
anything derived from the device result).  The K-column comparisons are bit for bit."""
import ctypes

import numpy as np
import pytest

import patch_gs_model as gm
import patch_schwarz_model as pm
from test_gpu_patch_multi import sweeps_multi
from test_gpu_patch_schwarz import ALPHA, EPS, Case, check_sweeps, sweeps_dev

pytestmark = pytest.mark.gpu

S = 2   # sweeps of every run: one launch in every family
BTD_FORMS = [(m, "row") for m in range(2, 10)] + [(m, "dense") for m in range(1, 6)]      # btd_form
PATCH_FORMS = [(m, "row") for m in range(2, 9)] + [(m, "dense") for m in range(1, 6)]     # patch_form
MULTI_FORMS = [(2, "row"), (4, "row"), (2, "dense")]                                       # multi_form
KCS = (1, 2, 3, 5, 8)   # column groups 1, 2, 4, 8, 8


def test_the_lists_have_the_sizes_of_the_header():
    assert (len(BTD_FORMS), len(PATCH_FORMS), len(MULTI_FORMS)) == (13, 12, 3)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def lists(m, ne):
    """contiguous index lists of ne blocks of m rows (1-based, m x ne)"""
    return np.arange(ne, dtype=np.int64)[None, :] * m + np.arange(1, m + 1, dtype=np.int64)[:, None]


def btd_owned(m, halo):
    """BtdTile<M, CMP> (aggmg_hip.hip): 256 threads, NS slabs of 256 / m elements; a launch that keeps `halo` elements a
    side owns the rest (fused_tile_plan without a restriction)"""
    ns = {1: 2, 2: 1, 3: 3, 4: 2}.get(m, 3 if m <= 7 else 2)
    return (256 // m) * ns - 2 * halo


def bound(u_ref, u0, d_ref):
    base = 64 * EPS * S * max(np.max(np.abs(u_ref)), np.max(np.abs(u0)), 1e-300)
    return (base if d_ref <= base else 4 * d_ref), base


# ---- the fused block-tridiagonal family ------------------------------------------------------------------------------------
def jacobi_model(T, u, b, w):
    """block-Jacobi sweeps in float64, vectorised over the elements"""
    for _ in range(S):
        r = (b - T.matvec(u)).reshape(T.ne, T.m)
        u = u + w * np.linalg.solve(T.diag, r[:, :, None])[:, :, 0].reshape(-1)
    return u


@pytest.mark.parametrize("m,coupling", BTD_FORMS)
def test_block_jacobi_launches_every_form(mg, oracle, m, coupling):
    for ne in (3, btd_owned(m, S) + 1):
        T = pm.random_block_tridiag(m, ne, coupling, 300 + 7 * m + ne)
        A = T.tocsc()
        op = mg.DeviceOperator(A)
        sm = mg.BlockJacobi(op, lists(m, ne))
        try:
            assert sm.structured, (m, coupling, ne)
            N = m * ne
            u0, b = oracle.splitmix_normal(N, 11 + ne), oracle.splitmix_normal(N, 13 + ne)
            ud = sweeps_dev(mg, op, sm, u0, b, ALPHA, S)
            So = oracle.BlockJacobi([oracle.LU(T.diag[e]) for e in range(ne)], lists(m, ne))
            ur = u0
            for _ in range(S):
                ur = oracle.smooth_once(So, A, ur, b, ALPHA)
            d_ref = float(np.max(np.abs(ur - jacobi_model(T, u0, b, ALPHA))))
            tol, base = bound(ur, u0, d_ref)
            d = float(np.max(np.abs(ud - ur)))
            print(f"m {m} {coupling} ne {ne}: device-oracle {d:.3e}  oracle-model {d_ref:.3e}  bound {base:.3e}")
            assert d <= tol, (m, coupling, ne, d, tol)
        finally:
            sm.free()
            op.free()


def test_block_jacobi_off_the_list_takes_the_generic_route(mg, oracle):
    """dense couplings with 6 rows per element: the first form off btd_form.  The generic route of the comparison: the same
    blocks listed in a scrambled order, which no structured form serves"""
    m = 6
    for ne in (3, btd_owned(5, S) + 1):
        T = pm.random_block_tridiag(m, ne, "dense", 900 + ne)
        A = T.tocsc()
        op, op_g = mg.DeviceOperator(A), mg.DeviceOperator(A)
        sm = mg.BlockJacobi(op, lists(m, ne))
        sg = mg.BlockJacobi(op_g, np.ascontiguousarray(lists(m, ne)[:, np.random.default_rng(ne).permutation(ne)]))
        try:
            assert not sm.structured and not sg.structured
            N = m * ne
            u0, b = oracle.splitmix_normal(N, 17 + ne), oracle.splitmix_normal(N, 19 + ne)
            ud, ug = sweeps_dev(mg, op, sm, u0, b, ALPHA, S), sweeps_dev(mg, op_g, sg, u0, b, ALPHA, S)
            assert np.array_equal(ud, ug), (ne, float(np.max(np.abs(ud - ug))))
            um = jacobi_model(T, u0, b, ALPHA)   # (and both are the sweeps)
            assert np.max(np.abs(ud - um)) <= 64 * EPS * S * max(np.max(np.abs(um)), np.max(np.abs(u0)))
        finally:
            for x in (sm, sg, op, op_g):
                x.free()


# ---- the element-patch family ----------------------------------------------------------------------------------------------
def patch_owned(mg, m, multiplicative):
    lib = mg.default_context().lib
    te, own, halo, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    if multiplicative:
        assert lib.aggmg_patch_gs_tile_plan(m, S, ctypes.byref(te), ctypes.byref(own), ctypes.byref(halo), ctypes.byref(smax)) == 0
    else:
        assert lib.aggmg_patch_tile_plan(m, S, ctypes.byref(te), ctypes.byref(own), ctypes.byref(smax)) == 0
    assert own.value >= 1 and smax.value >= S
    return own.value


@pytest.mark.parametrize("m,coupling", PATCH_FORMS)
def test_patch_schwarz_launches_every_form(mg, oracle, m, coupling):
    for ne in (3, patch_owned(mg, m, False) + 1):
        T = pm.random_block_tridiag(m, ne, coupling, 500 + 7 * m + ne)
        u0, b = oracle.splitmix_normal(m * ne, 23 + ne), oracle.splitmix_normal(m * ne, 29 + ne)
        for hybrid in (True, False):
            C = Case(mg, T, hybrid)
            try:
                assert C.fused.fused, (m, coupling, ne, hybrid)
                check_sweeps(mg, C, u0, b, ALPHA, S, f"m {m} {coupling} ne {ne} hybrid {hybrid}")
            finally:
                C.free()


@pytest.mark.parametrize("m,coupling", PATCH_FORMS)
def test_patch_gauss_seidel_launches_every_form(mg, oracle, m, coupling):
    """(the multiplicative smoother has no generic route: its reference is the float64 model of tests/patch_gs_model.py, whose
    own distance is the one to the same sweeps in np.longdouble, as in tests/test_gpu_patch_gs.py)"""
    for ne in (3, patch_owned(mg, m, True) + 1):
        T = pm.random_block_tridiag(m, ne, coupling, 700 + 7 * m + ne)
        u0, b = oracle.splitmix_normal(m * ne, 31 + ne), oracle.splitmix_normal(m * ne, 37 + ne)
        op = mg.DeviceOperator(T.tocsc())
        G = mg.ElementPatchGaussSeidel(op, m, ne)
        try:
            assert G.fused and G.kind == 3, (m, coupling, ne)
            ud = sweeps_dev(mg, op, G, u0, b, ALPHA, S)
            um = gm.gs_sweeps(T, u0, b, [ALPHA] * S, False)
            d_ref = float(np.max(np.abs(um - gm.gs_sweeps(T, u0, b, [ALPHA] * S, False, dtype=np.longdouble))))
            tol, base = bound(um, u0, d_ref)
            d = float(np.max(np.abs(ud - um)))
            print(f"m {m} {coupling} ne {ne}: device-model {d:.3e}  model-longdouble {d_ref:.3e}  bound {base:.3e}")
            assert d <= tol, (m, coupling, ne, d, tol)
        finally:
            G.free()
            op.free()


def test_patch_off_the_list_is_not_fused(mg):
    T = pm.random_block_tridiag(9, 4, "row", 3)
    op = mg.DeviceOperator(T.tocsc())
    P = mg.ElementPatchSchwarz(op, 9, 4)
    assert not P.fused
    P.free()
    op.free()


# ---- the K-column family ---------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def multi_owned(mg, m, kb):
    te, own, halo, smax = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib = mg.default_context().lib
    assert lib.aggmg_patch_gs_multi_tile_plan(m, S, kb, ctypes.byref(te), ctypes.byref(own), ctypes.byref(halo), ctypes.byref(smax)) == 0
    assert own.value >= 1 and smax.value >= S
    return own.value


@pytest.mark.parametrize("m,coupling", MULTI_FORMS)
def test_smooth_multi_is_single_column_sweeps(mg, oracle, m, coupling):
    assert {multi_owned(mg, m, kb) for kb in (1, 2, 4, 8)} == {multi_owned(mg, m, 8)}   # (the tile does not depend on the group)
    for ne in (3, multi_owned(mg, m, 8) + 1):
        T = pm.random_block_tridiag(m, ne, coupling, 1100 + 7 * m + ne)
        N = m * ne
        op = mg.DeviceOperator(T.tocsc())
        G = mg.ElementPatchGaussSeidel(op, m, ne)
        try:
            assert G.fused and G.kind == 3
            U0 = np.column_stack([oracle.splitmix_normal(N, 40 + 3 * j + ne) for j in range(max(KCS))])
            B = np.column_stack([oracle.splitmix_normal(N, 70 + 5 * j + ne) for j in range(max(KCS))])
            R = np.column_stack([sweeps_dev(mg, op, G, U0[:, j].copy(), B[:, j].copy(), ALPHA, S) for j in range(max(KCS))])
            um = gm.gs_sweeps(T, U0[:, 0], B[:, 0], [ALPHA] * S, False)   # (equal to a WRONG single run cannot pass)
            assert np.max(np.abs(R[:, 0] - um)) <= 64 * EPS * S * max(np.max(np.abs(um)), np.max(np.abs(U0[:, 0])))
            for kc in KCS:
                X = sweeps_multi(G, U0, B, [ALPHA] * S, False, N, kc)
                for j in range(kc):
                    assert _same(X[:, j], R[:, j]), (m, coupling, ne, kc, j, float(np.max(np.abs(X[:, j] - R[:, j]))))
        finally:
            G.free()
            op.free()


@pytest.mark.parametrize("m,coupling", MULTI_FORMS)
def test_residual_multi_is_single_column_residuals(mg, oracle, m, coupling):
    c = mg.default_context()
    for ne in (3, 256 // m - 2 + 1):   # (btd_residual_multi_kernel: 256 / m elements a tile, one of halo a side)
        T = pm.random_block_tridiag(m, ne, coupling, 1300 + 7 * m + ne)
        N = m * ne
        op = mg.DeviceOperator(T.tocsc())
        sm = mg.BlockJacobi(op, lists(m, ne))   # (set-up gives the operator its block-tridiagonal form)
        try:
            assert sm.structured
            rd, wr = op.residual_multi_launch_bytes(1)   # the K-column kernel covers the operator
            assert rd > 0 and wr == 8 * N
            X = np.column_stack([oracle.splitmix_normal(N, 90 + 3 * j + ne) for j in range(max(KCS))])
            B = np.column_stack([oracle.splitmix_normal(N, 110 + 5 * j + ne) for j in range(max(KCS))])
            R = np.empty_like(X)
            for j in range(max(KCS)):
                dx, db, dr = c.to_device(X[:, j]), c.to_device(B[:, j]), c.alloc(N)
                c.check(c.lib.aggmg_residual_dev(c.handle, op.handle, dx.ptr, db.ptr, dr.ptr))
                R[:, j] = dr.download()
                for v in (dx, db, dr):
                    v.free()
            for kc in KCS:
                dX, dB = c.to_device(X[:, :kc].ravel(order="F")), c.to_device(B[:, :kc].ravel(order="F"))
                dR = c.to_device(np.full(N * kc, np.nan))
                op.residual_multi_dev(dX, dB, dR, kc, N)
                got = dR.download().reshape((N, kc), order="F")
                for v in (dX, dB, dR):
                    v.free()
                for j in range(kc):
                    assert _same(got[:, j], R[:, j]), (m, coupling, ne, kc, j, float(np.max(np.abs(got[:, j] - R[:, j]))))
        finally:
            sm.free()
            op.free()
