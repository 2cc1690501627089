"""Direct solves of CG operators on the device, in element-chain order (AGGMG_COARSE_DEVICE_CHAIN; csrc/setup.hip
setup_cr_chain, cr_pack_chain_kernel; the gather / scatter of csrc/cr_kernels.hpp).  A CG operator in the reference's
vertices-first numbering has no band; in the order [left vertex, interior nodes] of every element it is block-tridiagonal
with p x p blocks, which the block cyclic reduction of the coarsest solve factors as it factors a DG operator.

What is asserted is the normwise backward error

    eta(x) = ||b - A x||_2 / (||A||_inf ||x||_2 + ||b||_2)

against that of SciPy's SuperLU on the same matrix and right-hand side: eta_dev <= R max(eta_LU, 2^-53).  A residual
bound relative to ||b|| (tests/test_gpu_coarse_cr.py: 1e-12) cannot be used on these operators -- their solutions are
large against b, and SuperLU itself misses it from about 10^3 elements on; the two SOLUTIONS differ by cond(A) eps.
R = 4 x the largest ratio measured over all cases of this file, rounded up to a power of two (profiles/
r17_chain_direct.md); a packing or permutation mistake gives eta of 1e-3 .. 1."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

# largest eta_dev / max(eta_LU, 2^-53) measured: see profiles/r17_chain_direct.md
R = 4.0


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


@pytest.fixture(scope="module")
def lib():
    from agglomerationmultigrid1d_amd import _lib
    return _lib


def device_memory():
    from agglomerationmultigrid1d_amd.api import device_memory
    return device_memory()


def eta(A, x, b):
    return np.linalg.norm(b - A @ x) / (abs(A).sum(axis=1).max() * np.linalg.norm(x) + np.linalg.norm(b))


BCS = {"neu-dir": None,   # the model problem's
       "dir-neu": (("dir", 1.0), ("neu", -np.sin(1.0))),
       "dir-dir": (("dir", 1.0), ("dir", np.cos(1.0)))}


@functools.lru_cache(maxsize=None)
def cg_case(n, p, bc="neu-dir"):
    """operator, its own right-hand side, element lists (1-based, (p + 1) x n), a seeded random right-hand side and
    SuperLU's solutions of both with their backward errors -- computed once per shape, read-only afterwards"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(n, ps=(p,), bc=BCS[bc])
    A = sp.csc_matrix(U.A[0])
    rhs = [np.asarray(U.b, dtype=np.float64), np.random.default_rng(1000 * p + n).standard_normal(A.shape[0])]
    lu = spla.splu(A)
    ref = [lu.solve(b) for b in rhs]
    for v in rhs + ref:
        v.setflags(write=False)
    return dict(A=A, elems=U.element_nodes(0), rhs=rhs, ref=ref, eta_lu=[eta(A, x, b) for x, b in zip(ref, rhs)])


def one_level(mg, lib, A, elems=None, mode=None):
    """-> (ctx, H, keep): a one-level hierarchy IS the direct solve; elems: the chain form comes from a point-Jacobi
    smoother given the element lists (it may go once the hierarchy stands: the hierarchy shares the form)"""
    ctx = mg.default_context()
    op = mg.DeviceOperator(A, lib.OP_STIFFNESS, ctx)
    S = mg.JacobiSmoother(op, ctx, elems) if elems is not None else None
    assert S is None or S.structured
    H = mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=False,
                         coarse_mode=lib.COARSE_DEVICE_CHAIN if mode is None else mode)
    return ctx, H, (op, S)


def solve(ctx, H, b):
    N = len(b)
    xd = ctx.alloc(N)
    H.vcycle_dev(ctx.to_device(np.zeros(N)), ctx.to_device(b), xd, 0, 0, 1.0)
    return xd.download()


def check_eta(A, x, b, eta_lu, what):
    e = eta(A, x, b)
    ratio = e / max(eta_lu, 2.0 ** -53)
    print(f"{what}: eta_dev {e:.3e}  eta_LU {eta_lu:.3e}  ratio {ratio:.3f}")
    assert e <= R * max(eta_lu, 2.0 ** -53), (what, e, eta_lu)


def check_route(H, p):
    info = H.coarse_info()
    assert info["on_device"] and info["block_size"] == p and info["order"] == "element chain", info
    assert 0.0 <= info["probe_backward_error"] < 1e-10, info
    return info


CASES = [(1, 2), (2, 3), (8, 2), (33, 3), (64, 4), (16, 8),       # tail only
         (2100, 2), (1100, 4), (600, 8),                          # one chunk stage
         (33000, 4)]                                              # stage with stack


@pytest.mark.parametrize("n,p", CASES)
def test_chain_order_solve_from_the_element_lists(mg, lib, n, p):
    c = cg_case(n, p)
    A = c["A"]
    ctx, H, keep = one_level(mg, lib, A, c["elems"])
    check_route(H, p)
    xs = []
    for k, (b, e_lu) in enumerate(zip(c["rhs"], c["eta_lu"])):
        xs.append(solve(ctx, H, b))
        check_eta(A, xs[-1], b, e_lu, f"n={n} p={p} rhs {k}")
    # the handle again: the first right-hand side after the second, bit for bit
    assert np.array_equal(solve(ctx, H, c["rhs"][0]), xs[0])
    H.free()


@pytest.mark.parametrize("bc", ["dir-neu", "neu-dir", "dir-dir"])
@pytest.mark.parametrize("n,p", [(64, 4), (1100, 4)])
def test_boundary_rows(mg, lib, n, p, bc):
    c = cg_case(n, p, bc)
    ctx, H, keep = one_level(mg, lib, c["A"], c["elems"])
    check_route(H, p)
    for k, (b, e_lu) in enumerate(zip(c["rhs"], c["eta_lu"])):
        check_eta(c["A"], solve(ctx, H, b), b, e_lu, f"n={n} p={p} {bc} rhs {k}")
    H.free()


@pytest.mark.parametrize("n,p", [(64, 4), (1100, 4), (8, 2)])
def test_chain_form_detected_from_the_operator_alone(mg, lib, n, p):
    c = cg_case(n, p)
    ctx, H, keep = one_level(mg, lib, c["A"])          # no smoother, no lists: AGGMG_OPT_DETECT_CHAIN
    check_route(H, p)
    for k, (b, e_lu) in enumerate(zip(c["rhs"], c["eta_lu"])):
        check_eta(c["A"], solve(ctx, H, b), b, e_lu, f"detected n={n} p={p} rhs {k}")
    # the same bits as with the lists: the two chain forms are the same arrays
    ctx2, H2, keep2 = one_level(mg, lib, c["A"], c["elems"])
    assert np.array_equal(solve(ctx, H, c["rhs"][1]), solve(ctx2, H2, c["rhs"][1]))
    H.free(), H2.free()
    was = ctx.option(lib.OPT_DETECT_CHAIN, 1)
    before = device_memory()
    ctx.set_option(lib.OPT_DETECT_CHAIN, 0)
    try:
        op = mg.DeviceOperator(c["A"], lib.OP_STIFFNESS, ctx)
        held = device_memory()
        with pytest.raises(lib.UnsupportedError, match="no element-chain form"):
            mg.MeshHierarchy(None, [op], [], [], ctx=ctx, coarse_mode=lib.COARSE_DEVICE_CHAIN)
        assert device_memory() == held
        op.free()
    finally:
        ctx.set_option(lib.OPT_DETECT_CHAIN, was)
    assert device_memory() == before


def test_numbering_that_is_not_vertices_first(mg, lib):
    n, p = 64, 4
    c = cg_case(n, p)
    A, N = c["A"], c["A"].shape[0]
    perm = np.random.default_rng(17).permutation(N)              # new number of old node i: perm[i]
    P = sp.csr_matrix((np.ones(N), (perm, np.arange(N))), shape=(N, N))
    As = sp.csc_matrix(P @ A @ P.T)
    elems = perm[c["elems"] - 1] + 1
    ctx, H, keep = one_level(mg, lib, As, elems)
    check_route(H, p)
    ctx0, H0, keep0 = one_level(mg, lib, A, c["elems"])
    lu = spla.splu(As)
    for k, b in enumerate(c["rhs"]):
        bs = P @ b
        xs = solve(ctx, H, bs)
        check_eta(As, xs, bs, eta(As, lu.solve(bs), bs), f"scrambled numbering rhs {k}")
        x = solve(ctx0, H0, b)
        assert np.linalg.norm(xs[perm] - x) <= 1e-9 * np.linalg.norm(x)
    H.free(), H0.free()


def block_tridiag(nb, m, seed):
    """random block-tridiagonal, block-diagonally dominant: a DG-shaped operator, no element chain"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dr, dc, cnt, shift in ((0, 0, nb, 4.0 * m), (1, 0, nb - 1, 0.0), (0, 1, nb - 1, 0.0)):
        blk = rng.standard_normal((cnt, m, m)) + shift * np.eye(m)
        e = np.arange(cnt)
        rows.append(((e + dr)[:, None, None] * m + ii).ravel())
        cols.append(((e + dc)[:, None, None] * m + jj).ravel())
        vals.append(blk.ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nb * m, nb * m))


def test_refusals_name_the_reason_and_hold_no_memory(mg, lib, oracle):
    ctx = mg.default_context()
    # block-tridiagonal DG-shaped operators with 4 x 4 blocks: N = 104, and N = 101 -- the size of a CG operator of degree
    # 4 on 25 elements, but with twice its entries
    for A in (block_tridiag(26, 4, 3), block_tridiag(30, 4, 4)[:101, :101].tocsc()):
        op = mg.DeviceOperator(A, lib.OP_STIFFNESS, ctx)
        held = device_memory()
        with pytest.raises(lib.UnsupportedError, match="no element-chain form"):
            mg.MeshHierarchy(None, [op], [], [], ctx=ctx, coarse_mode=lib.COARSE_DEVICE_CHAIN)
        assert device_memory() == held
        # ... which the cyclic reduction in the operator's own order takes
        H = mg.MeshHierarchy(None, [op], [], [], ctx=ctx, coarse_mode=lib.COARSE_DEVICE_CR)
        assert H.coarse_info()["order"] == "operator" and H.coarse_info()["on_device"]
        H.free()
    # CG p = 9: blocks of 9 rows
    o = oracle
    mesh, bd = o.model_problem(8)
    cg = o.CgMesh(mesh, 9)
    A9, _ = o.cg_stiffness_and_rhs(cg, mesh, np.cos, bd)
    elems = np.array([el.mNodesInd for el in cg.mElements], dtype=np.int64).T
    op = mg.DeviceOperator(A9, lib.OP_STIFFNESS, ctx)
    S = mg.JacobiSmoother(op, ctx, elems)
    assert not S.structured
    held = device_memory()
    with pytest.raises(lib.UnsupportedError, match="m > 8"):
        mg.MeshHierarchy(None, [op], [], [], ctx=ctx, coarse_mode=lib.COARSE_DEVICE_CHAIN)
    assert device_memory() == held


def test_auto_takes_the_chain_only_where_the_host_solver_refuses_the_band(mg, lib):
    # CG p = 2 on 16384 elements, N = 32769: band storage 3 * 16384 * N * 8 bytes = 1.3e10 > 8e9
    c = cg_case(16384, 2)
    ctx, H, keep = one_level(mg, lib, c["A"], mode=lib.COARSE_AUTO)
    check_route(H, 2)
    for k, (b, e_lu) in enumerate(zip(c["rhs"], c["eta_lu"])):
        check_eta(c["A"], solve(ctx, H, b), b, e_lu, f"AUTO n=16384 p=2 rhs {k}")
    H.free()
    # CG p = 4 on 64 elements: the host banded LU takes it, as before
    c = cg_case(64, 4)
    ctx, H, keep = one_level(mg, lib, c["A"], c["elems"], mode=lib.COARSE_AUTO)
    info = H.coarse_info()
    assert not info["on_device"] and info["order"] == "operator" and info["block_size"] == 0, info
    H.free()


@pytest.mark.parametrize("K", [3, 11])
def test_columns_are_the_single_column_solves(mg, lib, K):
    n, p = 1100, 4
    c = cg_case(n, p)
    A, N = c["A"], c["A"].shape[0]
    ctx, H, (op, S) = one_level(mg, lib, A, c["elems"])
    B = np.random.default_rng(K).standard_normal((N, K))
    B[:, 0] = c["rhs"][0]
    if K > 2:
        B[:, 2] = 0.0
    dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
    dB.upload(B)
    H.coarse_solve_multi_dev(dB, dX)
    X = dX.download()
    for j in range(K):
        assert np.array_equal(X[:, j], solve(ctx, H, B[:, j])), (K, j)
    assert not X[:, 2].any()
    assert np.array_equal(dB.download(), B)
    check_eta(A, X[:, 0], B[:, 0], c["eta_lu"][0], f"K={K} column 0")
    # the direct solver of the operator: the same route, the same bits
    ds = mg.DirectSolver(op)
    assert ds.where == "device (element chain)"
    dU = ds.solve_dev(dB)
    assert isinstance(dU, mg.DeviceMatrix) and np.array_equal(dU.download(), X)
    assert np.array_equal(ds.solve_dev(ctx.to_device(B[:, 1])).download(), X[:, 1])
    H.free()


def test_err_histories_of_cg_hierarchies_come_from_the_device(mg, lib, oracle):
    o = oracle
    Hc, bc = o.build_cg_hierarchy(32, ps=(4, 2, 1), nDG=1)
    Hg = mg.MeshHierarchy.from_reference(Hc)
    _, ito, _, erro = o.multigrid(Hc, np.zeros(len(bc)), bc, 60, 1e-9)
    _, itg, _, errg = mg.multigrid(Hg, np.zeros(len(bc)), bc, 60, 1e-9)
    assert Hg._direct_solver.where == "device (element chain)"
    assert itg == ito and np.allclose(errg, erro, rtol=1e-6, atol=1e-9 * erro[0])
    # the stationary loop on the level-0 CG operator, point Jacobi
    A, cgm = Hc.mStiffness[0], Hc.mMeshes[0]
    u0 = np.zeros(len(bc))
    _, ito, _, erro = o.iterative_smoother_solve(A, o.cg_smoother(cgm, A, 'jac'), u0, bc, maxiter=40, tol=1e-30, alpha=2.0 / 3.0)
    Sg = mg.cg_smoother(cgm, A, 'jac')
    _, itg, _, errg = mg.iterative_smoother_solve(A, Sg, u0, bc, maxiter=40, tol=1e-30, alpha=2.0 / 3.0)
    assert Sg._direct_solver.where == "device (element chain)"
    assert itg == ito == 40 and np.allclose(errg, erro, rtol=1e-6, atol=1e-9 * erro[0])


def test_multigrid_with_err_history_at_4096_elements(mg, lib):
    """the size at which the host banded LU of the fine operator (N = 16385, half-width 12288) is an O(N^3) factorisation"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, build_device_cg_hierarchy
    U = UniformCgDgHierarchy(4096)
    H = build_device_cg_hierarchy(U)
    b = np.asarray(U.rhs(), dtype=np.float64)
    x, it, res, err = mg.multigrid(H, np.zeros(len(b)), b, 12, 1e-8)
    assert H._direct_solver.where == "device (element chain)"
    assert len(err) == len(res) == it and it >= 2
    assert all(e1 < e0 for e0, e1 in zip(err, err[1:])), err


def test_hierarchy_with_a_cg_coarsest_level(mg, lib, oracle):
    """tests/cg_heirarchy_test.jl cut short: CG p = 8 -> 4 -> 2, the coarsest level a CG level of degree 2"""
    o = oracle
    Ho, b = o.build_cg_hierarchy(64, ps=(8, 4, 2))
    H = mg.MeshHierarchy.from_reference(Ho, coarse_mode=lib.COARSE_DEVICE_CHAIN)
    check_route(H, 2)
    A = Ho.mStiffness[0]
    x0 = np.zeros(len(b))
    x, xr = x0, x0
    for cycle in range(3):
        x = mg.multigrid_v_cycle(H, x, b)
        xr = o.multigrid_v_cycle(Ho, xr, b)
        if cycle in (0, 2):
            assert np.linalg.norm(A @ (x - xr)) <= 1e-12 * np.linalg.norm(b)        # r0 = b: the zero initial guess
            assert np.linalg.norm(x - xr) < 1e-8 * np.linalg.norm(xr)


def test_device_memory_returns(mg, lib):
    c = cg_case(1100, 4)
    ctx, H, keep = one_level(mg, lib, c["A"], c["elems"])      # (the context's own work space is grown by now)
    solve(ctx, H, c["rhs"][0])
    H.free(), keep[1].free(), keep[0].free()
    before = device_memory()
    ctx, H, (op, S) = one_level(mg, lib, c["A"], c["elems"])
    N = c["A"].shape[0]
    solve(ctx, H, c["rhs"][0])
    dB, dX = mg.DeviceMatrix(ctx, N, 3), mg.DeviceMatrix(ctx, N, 3)
    H.coarse_solve_multi_dev(dB, dX)
    ctx.synchronize()
    held = device_memory()
    assert held[0] > before[0] and held[1] > before[1]
    H.free()
    after_h = device_memory()
    assert after_h[1] < held[1]
    S.free(), op.free()
    assert device_memory() == before
