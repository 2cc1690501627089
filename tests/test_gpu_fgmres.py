"""Flexible GMRES around the V-cycle on the device (aggmg_fgmres_dev, api.fgmres; EXTENSION) and the two streaming
passes of its orthogonalisation (aggmg_multi_dot_dev, aggmg_multi_axpy_norm_dev).

The passes are held to bits: dot i of the fused pass == aggmg_dot_dev of vector i, the norm the update pass returns ==
aggmg_norm2_dev of the vector it stored.  The update itself is nvec fused multiply-adds per entry, each with one
rounding of at most 2^-53 relative to its result: |w_new - (w + V c)| <= (nvec + 2) 2^-52 (|w| + |V||c|) componentwise
(the reference sum is formed in extended precision).

The solver is held to the NumPy model of the same algorithm on the oracle's cycle (tests/fgmres_model.py): iteration
counts to +-1 (round-off may move the last crossing by one, as for pcg), the true residual to 1.05 tol ||b||, and the
history entry by entry to rtol = max(1e-9, 10 d), d being the largest relative difference between the model's classical
and modified Gram-Schmidt histories of the same case -- a measure of how far round-off in the orthogonalisation alone
moves the history; the observed device-vs-model figures are in profiles/r20_fgmres.md."""
import ctypes
import gc

import numpy as np
import pytest

from fgmres_model import fgmres_model

pytestmark = pytest.mark.gpu

NS = [1, 7, 255, 256, 257, 4097, 1_000_003]
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


def _col_dot(ctx, V, i, ld, w, n):
    """aggmg_dot_dev on vector i of the device basis and w"""
    out = ctypes.c_double(0.0)
    ctx.check(ctx.lib.aggmg_dot_dev(ctx.handle, ctypes.c_void_p(V.ptr.value + 8 * i * ld), w.ptr, n, ctypes.byref(out)))
    return out.value


def _basis(ctx, mg, o, n, nvec, ld, seed):
    """(host V[n, nvec], device buffer of ld * nvec doubles with rows >= n of every column set to 1e300)"""
    Vh = o.splitmix_normal(n * nvec, seed).reshape(nvec, n).T
    buf = np.full((ld, nvec), 1e300, order="F")
    buf[:n, :] = Vh
    dV = mg.DeviceMatrix(ctx, ld, nvec)
    dV.upload(buf)
    return Vh, dV


# ---- 1. the fused dots, bit for bit ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pad", [(n, 0) for n in NS] + [(4097, 5)])
def test_multi_dot_is_dot_bit_for_bit(oracle, mg, n, pad):
    ctx = mg.default_context()
    nvecs = [k for k in (1, 2, 7, 8, 9, 17, 65) if n < 1_000_000 or k <= 17]
    ld = n + pad
    Vh, dV = _basis(ctx, mg, oracle, n, max(nvecs), ld, 5)
    wh = oracle.splitmix_normal(n, 6)
    dw = ctx.to_device(wh)
    ref = np.array([_col_dot(ctx, dV, i, ld, dw, n) for i in range(max(nvecs))])
    assert np.allclose(ref, Vh.T @ wh, rtol=0, atol=1e-13 * np.linalg.norm(wh) * np.linalg.norm(Vh, axis=0).max())
    if n == 4097:   # the same bits for a vector uploaded on its own (another address, another alignment)
        for i in (0, 3, 16):
            assert mg.dot(ctx.to_device(Vh[:, i]), dw) == ref[i]
    for nvec in nvecs:
        got = ctx.multi_dot(dV, dw, n=n, nvec=nvec, ld=ld)
        assert got.shape == (nvec,)
        assert np.array_equal(got, ref[:nvec]), (n, nvec, np.nonzero(got != ref[:nvec])[0][:5])
        assert np.array_equal(ctx.multi_dot(dV, dw, n=n, nvec=nvec, ld=ld), got)      # run to run
    assert np.array_equal(dw.download(), wh)


def test_multi_dot_arguments(oracle, mg):
    ctx = mg.default_context()
    dV = mg.DeviceMatrix(ctx, 8, 3)
    dw = ctx.alloc(8)
    with pytest.raises(mg.ArgumentError):
        ctx.multi_dot(dV, dw, n=8, nvec=0, ld=8)
    with pytest.raises(mg.ArgumentError):
        ctx.multi_dot(dV, dw, n=8, nvec=66, ld=8)
    with pytest.raises(mg.ArgumentError):
        ctx.multi_dot(dV, dw, n=8, nvec=3, ld=7)
    with pytest.raises(mg.ArgumentError):
        ctx.multi_axpy_norm(dV, np.ones(3), dV, n=8, nvec=3, ld=8)                   # w inside V
    assert np.array_equal(ctx.multi_dot(dV, dw, n=0, nvec=3, ld=8), np.zeros(3))     # no rows: empty sums


# ---- 2. the fused update with its norm -------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_multi_axpy_norm(oracle, mg, n):
    ctx = mg.default_context()
    ld = n + 5
    Vh, dV = _basis(ctx, mg, oracle, n, 17, ld, 7)
    wh = oracle.splitmix_normal(n, 8)
    for nvec in (1, 8, 9, 17):
        c = oracle.splitmix_normal(nvec, 20 + nvec)
        wbuf = np.concatenate([wh, np.full(5, -7.25)])          # five rows behind the vector: not the pass's to touch
        dw = ctx.to_device(wbuf)
        nrm = ctx.multi_axpy_norm(dV, c, dw, n=n, nvec=nvec, ld=ld)
        out = dw.download()
        got = out[:n]
        assert np.array_equal(out[n:], wbuf[n:])
        dn = ctx.to_device(got)
        assert nrm == mg.norm2(dn)                               # the norm of what was stored, bit for bit
        ref = wh.astype(np.longdouble) + Vh[:, :nvec].astype(np.longdouble) @ c.astype(np.longdouble)
        bound = (nvec + 2) * EPS * (np.abs(wh) + np.abs(Vh[:, :nvec]) @ np.abs(c))
        err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
        assert np.all(err <= bound), (n, nvec, float((err / bound).max()))
        # without the norm: the same vector
        dw2 = ctx.to_device(wbuf)
        assert ctx.multi_axpy_norm(dV, c, dw2, n=n, nvec=nvec, ld=ld, norm=False) is None
        assert np.array_equal(dw2.download(), out)
    # the basis and its padding rows were only read
    back = dV.download()
    assert np.array_equal(back[:n, :], Vh) and np.all(back[n:, :] == 1e300)


# ---- 3. the solver against the model ---------------------------------------------------------------------------------
_CASES = {}


def _hier(o, mg, name):
    """-> (Ho, H): oracle hierarchy and its device mirror, built once per module and never modified (the
    schedule test sets and clears its own weights)"""
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


def _true_residual(Ho, x, b):
    return float(np.linalg.norm(b - Ho.mStiffness[0] @ x))


@pytest.mark.parametrize("name,nPre,nPost,restart,tol", [("dg48", 2, 1, 30, 1e-8), ("dg48", 2, 1, 8, 1e-8),
                                                        ("dg128", 3, 3, 30, 1e-8), ("schwarz32", 3, 3, 10, 1e-10)])
def test_fgmres_against_the_model(oracle, mg, name, nPre, nPost, restart, tol):
    o = oracle
    Ho, H = _hier(o, mg, name)
    N = Ho.mStiffness[0].shape[0]
    b = o.splitmix_normal(N, 1)
    nb = np.linalg.norm(b)
    kw = dict(restart=restart, maxiter=200, tol=tol, nPre=nPre, nPost=nPost)
    _, itc, resc = fgmres_model(o, Ho, b, **kw)
    _, itm, resm = fgmres_model(o, Ho, b, mgs=True, **kw)
    k = min(itc, itm)
    d = float(np.max(np.abs(np.array(resc[:k]) - np.array(resm[:k])) / np.array(resc[:k])))
    rtol = max(1e-9, 10.0 * d)
    xg, itg, resg = mg.fgmres(H, b, **kw)
    assert len(resg) == itg
    k = min(itg, itc)
    seen = float(np.max(np.abs(np.array(resg[:k]) - np.array(resc[:k])) / np.array(resc[:k])))
    true = _true_residual(Ho, xg, b)
    print(f"fgmres {name} V({nPre},{nPost}) restart {restart}: iterations device {itg} model {itc} (mgs {itm}); "
          f"classical-vs-modified d = {d:.3e}, rtol = {rtol:.3e}, device-vs-model {seen:.3e} "
          f"(ratio to d {seen / d if d else float('inf'):.3g}); true residual / (tol ||b||) = {true / (tol * nb):.4f}, "
          f"last entry / (tol ||b||) = {resg[-1] / (tol * nb):.4f}")
    assert abs(itg - itc) <= 1
    assert all(resg[i + 1] <= resg[i] for i in range(itg - 1))
    assert true <= 1.05 * tol * nb
    assert seen <= rtol


# ---- 4. edges --------------------------------------------------------------------------------------------------------
def test_one_level_hierarchy_is_one_iteration(oracle, mg):
    Ho, _ = oracle.build_dg_agg_hierarchy(16, p=3, pAgg=1, nAgg=2, first=4)
    A = Ho.mStiffness[0]
    H = mg.MeshHierarchy(None, [A], [], [])
    b = oracle.splitmix_normal(A.shape[0], 1)
    x, it, res = mg.fgmres(H, b, tol=1e-10)
    assert it == 1 and len(res) == 1
    assert np.all(np.isfinite(x)) and np.isfinite(res[0])
    assert np.linalg.norm(b - A @ x) <= 1e-11 * np.linalg.norm(b)


def test_fgmres_edges(oracle, mg):
    o = oracle
    Ho, H = _hier(o, mg, "dg48")
    ctx = H.ctx
    N = Ho.mStiffness[0].shape[0]
    b = o.splitmix_normal(N, 1)
    nb = np.linalg.norm(b)
    x0 = o.splitmix_normal(N, 9)
    x0_copy = x0.copy()
    kw = dict(nPre=2, nPost=1)
    # maxiter = 0: nothing happens
    x, it, res = mg.fgmres(H, b, x0=x0, maxiter=0, **kw)
    assert it == 0 and res == [] and np.array_equal(x, x0)
    # warm start from a random guess
    xw, itw, resw = mg.fgmres(H, b, x0=x0, restart=30, maxiter=200, tol=1e-8, **kw)
    assert np.array_equal(x0, x0_copy)
    assert 0 < itw < 200 and resw[-1] < 1e-8 * nb
    assert _true_residual(Ho, xw, b) <= 1.05e-8 * nb
    # a guess already within the tolerance: untouched, no iteration
    x, it, res = mg.fgmres(H, b, x0=xw, restart=30, maxiter=200, tol=1e-7, **kw)
    assert it == 0 and res == [] and np.array_equal(x, xw)
    # restart 1: five entries that do not grow (nothing about convergence: short restarts stagnate on this cycle)
    x, it, res = mg.fgmres(H, b, restart=1, maxiter=5, tol=1e-8, **kw)
    assert it == 5 and len(res) == 5 and all(res[i + 1] <= res[i] for i in range(4))
    assert np.all(np.isfinite(x))
    # restart > maxiter: the one cycle is cut at maxiter, and x has its update
    x, it, res = mg.fgmres(H, b, restart=30, maxiter=4, tol=1e-8, **kw)
    assert it == 4 and all(res[i + 1] <= res[i] for i in range(3))
    assert abs(_true_residual(Ho, x, b) - res[-1]) <= 1e-6 * res[-1]
    _, _, resm = fgmres_model(o, Ho, b, restart=30, maxiter=4, tol=1e-8, **kw)
    assert np.allclose(res, resm, rtol=1e-9)
    # DeviceVectors in, a DeviceVector out: the same bits as the host-array call, inputs untouched
    xh, ith, resh = mg.fgmres(H, b, x0=x0, restart=8, maxiter=20, tol=1e-8, **kw)
    db, d0 = ctx.to_device(b), ctx.to_device(x0)
    xd, itd, resd = mg.fgmres(H, db, x0=d0, restart=8, maxiter=20, tol=1e-8, **kw)
    assert isinstance(xd, mg.DeviceVector) and itd == ith and resd == resh
    assert np.array_equal(xd.download(), xh)
    assert np.array_equal(db.download(), b) and np.array_equal(d0.download(), x0)
    xz, itz, resz = mg.fgmres(H, db, restart=8, maxiter=20, tol=1e-8, **kw)           # x0 None on the device: zeros
    assert (itz, resz) == mg.fgmres(H, b, restart=8, maxiter=20, tol=1e-8, **kw)[1:]
    # argument errors, before anything runs
    for bad in (0, 65):
        with pytest.raises(mg.ArgumentError):
            mg.fgmres(H, b, restart=bad, **kw)
    with pytest.raises(mg.ArgumentError):
        mg.fgmres(H, b, maxiter=-1, **kw)
    with pytest.raises(mg.ArgumentError, match="K right-hand sides"):
        mg.fgmres(H, np.stack([b, b], axis=1), **kw)
    with pytest.raises(mg.ArgumentError, match="K right-hand sides"):
        mg.fgmres(H, mg.DeviceMatrix(ctx, N, 2), **kw)
    hist = np.zeros(4)
    it = ctypes.c_int(0)
    with pytest.raises(mg.ArgumentError, match="alias"):                              # x aliasing b
        ctx.check(ctx.lib.aggmg_fgmres_dev(ctx.handle, H.handle, db.ptr, db.ptr, 8, 4, 1e-8, 2, 1, 2.0 / 3.0,
                                           hist.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(it)))
    assert np.array_equal(db.download(), b)


def test_fgmres_with_an_unsymmetric_sweep_schedule(oracle, mg):
    """level 0 smooths with pre = (0.9, 0.55), post = (0.5, 0.8): post is not pre reversed, the cycle is no symmetric
    preconditioner, and the minimal-residual loop converges all the same"""
    o = oracle
    Ho, H = _hier(o, mg, "dg48")
    b = o.splitmix_normal(Ho.mStiffness[0].shape[0], 1)
    nb = np.linalg.norm(b)
    try:
        H.set_sweep_weights(0, [0.9, 0.55], [0.5, 0.8])
        x, it, res = mg.fgmres(H, b, restart=30, maxiter=200, tol=1e-8, nPre=2, nPost=2)
    finally:
        H.clear_sweep_weights()
    assert 0 < it < 200 and res[-1] < 1e-8 * nb
    assert all(res[i + 1] <= res[i] for i in range(it - 1))
    assert _true_residual(Ho, x, b) <= 1.05e-8 * nb


# ---- 5. several workgroups per vector --------------------------------------------------------------------------------
def test_fgmres_on_a_uniform_hierarchy(mg):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    ctx = mg.default_context()
    U = UniformDgAggHierarchy(2 ** 14, p=3, pAgg=1, ratios=(4, 2, 2))
    H = build_device_hierarchy(U, ctx)
    b = U.rhs()
    nb = np.linalg.norm(b)
    x, it, res = mg.fgmres(H, b, restart=30, maxiter=200, tol=1e-8, nPre=2, nPost=1)
    assert 0 < it < 200 and res[-1] < 1e-8 * nb
    assert all(res[i + 1] <= res[i] for i in range(it - 1))
    assert np.linalg.norm(mg.residual(H._ops[0], x, b)) <= 1.05e-8 * nb
    x2, it2, res2 = mg.fgmres(H, b, restart=30, maxiter=200, tol=1e-8, nPre=2, nPost=1)
    assert it2 == it and res2 == res and np.array_equal(x2, x)


# ---- 6. the work space belongs to the context ------------------------------------------------------------------------
def test_fgmres_work_space_lifetime(oracle, mg):
    from agglomerationmultigrid1d_amd import api
    Ho, _ = oracle.build_dg_agg_hierarchy(48, p=3, pAgg=1, nAgg=3, first=4)
    N = Ho.mStiffness[0].shape[0]
    b = oracle.splitmix_normal(N, 1)
    gc.collect()
    start = api.device_memory()
    ctx = mg.Context(0)
    try:
        H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
        built = api.device_memory()[1]
        mg.fgmres(H, b, restart=6, maxiter=12, tol=1e-8, nPre=2, nPost=1)
        m6 = api.device_memory()[1]
        assert m6 - built >= (2 * 6 + 2) * N * 8                 # the work space (and the cycle's own scratch)
        mg.fgmres(H, b, restart=6, maxiter=12, tol=1e-8, nPre=2, nPost=1)
        assert api.device_memory()[1] == m6                      # kept, nothing more
        mg.fgmres(H, b, restart=9, maxiter=12, tol=1e-8, nPre=2, nPost=1)
        assert api.device_memory()[1] - m6 == 2 * 3 * N * 8      # exchanged for the other size
        mg.fgmres(H, b, restart=2, maxiter=12, tol=1e-8, nPre=2, nPost=1)
        assert api.device_memory()[1] - m6 == -2 * 4 * N * 8
        # the hierarchy gives back what it took; what is left belongs to the context: the work space among it
        H.free()
        for obj in list(H.mSmoothers) + H._ops + H._Ls:
            obj.free()
        gc.collect()
        assert api.device_memory()[1] - start[1] >= (2 * 2 + 2) * N * 8
    finally:
        ctx.close()
    gc.collect()
    assert api.device_memory() == start
