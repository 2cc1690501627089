"""The coarsest direct solve of a column group in one launch sequence (cr_solve_cols / cr_walk in csrc/aggmg_hip.hip, the column
dimension of csrc/cr_kernels.hpp; C ABI aggmg_hier_coarse_solve_multi_dev; EXTENSION: the reference's `A_n \\ rhs_n`,
src/solvers.jl:39, takes one vector per cycle).  The contract is bitwise: column j of the batched solve is the single-column
solve of column j -- every column keeps the single-column arithmetic, only the launches are shared -- on every path of the
solver: one chunk stage + register-blocked tail (block size 4), stage + parallel-cyclic-reduction tail (block size 2), tail
only, scalar systems above and below the tail's row limit, a block count that is no power of two, and a system whose last
block is incomplete (N not a multiple of the block size: the padded staging vectors).  K = 1, 3, 8, 9 (two groups), leading
dimensions N, N + 3 (columns off the 16-byte grid: staged) and N + 4 (in place), the rows between the columns untouched.

Through the public solvers on a 65536-element hierarchy (its coarsest system, 4096 blocks of 2, has a stage):
multigrid_v_cycle, pcg and multigrid on K = 8 columns against the single-vector calls, and the profiler's launch-scope count:
ONE (coarse, level) scope per group of a K-column cycle, where the column loop opened one per column."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

pytestmark = pytest.mark.gpu

KMAX = 9
KS = (1, 3, 8, 9)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    return mg.Context(0)


def block_tridiag(nb, m, seed, ragged=0):
    """random block-tridiagonal, block-diagonally dominant, not symmetric; ragged: that many trailing rows / columns dropped"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dr, dc, cnt, shift in ((0, 0, nb, 4.0 * m), (1, 0, nb - 1, 0.0), (0, 1, nb - 1, 0.0)):
        blk = rng.standard_normal((cnt, m, m)) + shift * np.eye(m)
        e = np.arange(cnt)
        rows.append(((e + dr)[:, None, None] * m + ii).ravel())
        cols.append(((e + dc)[:, None, None] * m + jj).ravel())
        vals.append(blk.ravel())
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nb * m, nb * m))
    N = nb * m - ragged
    return sp.csc_matrix(A[:N, :N])


def _uniform_level(n, p, ratios, level):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    return sp.csc_matrix(UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios).stiffness_csc(level))


def _scalar(oracle, n):
    Ho, _ = oracle.build_cg_hierarchy(n, ps=(4, 2, 1), nDG=1, pDG=0)      # config 5's shape: CG p = 4 -> 2 -> 1 -> DG p = 0
    return sp.csc_matrix(Ho.mStiffness[-1])


# name -> (matrix builder, block size, blocks, stages expected)
SHAPES = {
    "dg_p3_2048_elements": (lambda o: _uniform_level(2048, 3, (), 0), 4, 2048, True),          # 8192 rows: stage + tail
    "agg_4096_blocks_of_2": (lambda o: _uniform_level(65536, 3, (4, 2, 2), 3), 2, 4096, True),  # stage + (parallel) tail
    "agg_1024_blocks_of_2": (lambda o: _uniform_level(16384, 3, (4, 2, 2), 3), 2, 1024, False),  # tail only
    "scalar_5000": (lambda o: _scalar(o, 5000), 1, 5000, True),
    "scalar_1000": (lambda o: _scalar(o, 1000), 1, 1000, False),
    "random_3000_blocks_of_2": (lambda o: block_tridiag(3000, 2, 5), 2, 3000, True),            # no power of two
    "random_2999_and_a_half_blocks": (lambda o: block_tridiag(3000, 2, 6, ragged=1), 2, 3000, True),   # n0 M > N: staging
}


def _rhs(oracle, N):
    """a different seed per column; column 2 all zeros, column 5 a copy of column 1"""
    B = np.column_stack([oracle.splitmix_normal(N, 100 + j) for j in range(KMAX)])
    B[:, 2] = 0.0
    B[:, 5] = B[:, 1]
    return B


_cache = {}


def _case(mg, ctx, oracle, name):
    """the one-level hierarchy of a shape, its right-hand sides and the single-column solves of every column (computed
    once, shared by the tests, never modified)"""
    if name not in _cache:
        from agglomerationmultigrid1d_amd import _lib
        build, m, nb, staged = SHAPES[name]
        A = build(oracle)
        N = A.shape[0]
        op = mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx)
        H = mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_DEVICE_CR)
        info = H.coarse_info()
        assert info["on_device"] and info["block_size"] == m, info
        assert (N + m - 1) // m == nb
        assert (info["tail_blocks"] < nb) == staged, info      # the path the shape is here for
        B = _rhs(oracle, N)
        z = ctx.to_device(np.zeros(N))
        ref = np.empty((N, KMAX))
        for j in range(KMAX):
            x = ctx.alloc(N)
            H.vcycle_dev(z, ctx.to_device(B[:, j]), x, 0, 0, 1.0)      # a one-level cycle with 0 sweeps: the direct solve
            ref[:, j] = x.download()
        ref.setflags(write=False)
        B.setflags(write=False)
        _cache[name] = dict(A=A, N=N, H=H, op=op, B=B, ref=ref, info=info)
    return _cache[name]


def _upload(ctx, A, ld):
    N, K = A.shape
    pad = np.full((ld, K), np.nan, order="F")
    pad[:N] = A
    return ctx.to_device(pad.ravel(order="F"))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_batched_solve_is_the_single_column_solve(mg, ctx, oracle, name, K):
    c = _case(mg, ctx, oracle, name)
    H, N = c["H"], c["N"]
    dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
    dB.upload(c["B"][:, :K])
    H.coarse_solve_multi_dev(dB, dX)
    X = dX.download()
    for j in range(K):
        assert np.array_equal(X[:, j], c["ref"][:, j]), (name, K, j, float(np.max(np.abs(X[:, j] - c["ref"][:, j]))))
    if K > 2:
        assert not X[:, 2].any()                                  # the zero column
    if K > 5:
        assert np.array_equal(X[:, 5], X[:, 1])                   # copies agree bit for bit
    assert np.array_equal(dB.download(), c["B"][:, :K])           # B is left alone
    # run to run, and through the K-column cycle entry (a one-level cycle is the coarsest solve) and the direct solver
    dX2 = mg.DeviceMatrix(ctx, N, K)
    H.coarse_solve_multi_dev(dB, dX2)
    assert np.array_equal(dX2.download(), X)
    dX3 = mg.DeviceMatrix(ctx, N, K)
    H.vcycle_multi_dev(None, dB, dX3, nPre=0, nPost=0, alpha=1.0)
    assert np.array_equal(dX3.download(), X)


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_leading_dimension(mg, ctx, oracle, name, pad):
    """ld > N: the gap rows hold NaN in B and are untouched in X.  ld = N + 3 puts every other column off the 16 bytes the
    kernels' paired loads assume (the group goes through the staging vectors), ld = N + 4 keeps them on (in place)"""
    c = _case(mg, ctx, oracle, name)
    H, N = c["H"], c["N"]
    K, ld = KMAX, N + pad
    dB = _upload(ctx, c["B"], ld)
    dX = ctx.to_device(np.full(ld * K, np.nan))
    H.coarse_solve_multi_dev(dB, dX, K, ld)
    got = dX.download().reshape((ld, K), order="F")
    assert np.array_equal(got[:N], c["ref"]), (name, pad)
    assert np.isnan(got[N:]).all()


def test_against_sparse_lu(mg, ctx, oracle):
    """the backward-error bound tests/test_gpu_coarse_cr.py holds the single-column solve to"""
    c = _case(mg, ctx, oracle, "random_3000_blocks_of_2")
    assert c["info"]["tail"] == "parallel cyclic reduction", c["info"]      # cr_pcr_tail_kernel's column dimension
    A, N, K = c["A"], c["N"], 8
    dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
    dB.upload(c["B"][:, :K])
    c["H"].coarse_solve_multi_dev(dB, dX)
    X = dX.download()
    ref = spla.splu(A).solve(np.asarray(c["B"][:, :K]))
    for j in range(K):
        b = c["B"][:, j]
        assert np.linalg.norm(A @ X[:, j] - b) <= 1e-12 * np.linalg.norm(b), j
        assert np.linalg.norm(X[:, j] - ref[:, j]) <= 1e-11 * np.linalg.norm(ref[:, j]), j


def test_direct_solver_takes_matrices(mg, ctx, oracle):
    c = _case(mg, ctx, oracle, "dg_p3_2048_elements")
    ds = mg.DirectSolver(c["op"])
    assert ds.where == "device"
    N, K = c["N"], KMAX
    dB = mg.DeviceMatrix(ctx, N, K)
    dB.upload(c["B"])
    dU = ds.solve_dev(dB)
    assert isinstance(dU, mg.DeviceMatrix) and dU.shape == (N, K)
    U = dU.download()
    for j in range(K):
        uj = ds.solve_dev(ctx.to_device(c["B"][:, j]))
        assert isinstance(uj, mg.DeviceVector)
        assert np.array_equal(U[:, j], uj.download()), j
    assert np.array_equal(U, c["ref"])


def test_host_banded_lu_stays_column_by_column(mg, ctx, oracle):
    """cr.valid == false: the same bits as the single-column cycle"""
    from agglomerationmultigrid1d_amd import _lib
    A = block_tridiag(300, 2, 9)
    N, K = A.shape[0], 3
    op = mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx)
    H = mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_HOST_BANDED)
    assert not H.coarse_info()["on_device"]
    B = _rhs(oracle, N)[:, :K]
    dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
    dB.upload(B)
    H.coarse_solve_multi_dev(dB, dX)
    X = dX.download()
    z = ctx.to_device(np.zeros(N))
    for j in range(K):
        x = ctx.alloc(N)
        H.vcycle_dev(z, ctx.to_device(B[:, j]), x, 0, 0, 1.0)
        assert np.array_equal(X[:, j], x.download()), j
    H.free()


def _stage0_plan(mg, ctx, A):
    """(log2 chunk, blocks of stage 0's boundary system) of the one-level hierarchy of A, through aggmg_coarse_plan"""
    from agglomerationmultigrid1d_amd import _lib
    H = mg.MeshHierarchy(None, [mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx)], [], [], ctx=ctx, keep_host=False,
                         coarse_mode=_lib.COARSE_DEVICE_CR)
    q, nq, mb, nblk = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    ctx.check(ctx.lib.aggmg_coarse_plan(ctx.handle, H.handle, ctypes.byref(q), ctypes.byref(nq), ctypes.byref(mb),
                                        ctypes.byref(nblk)))
    return H, q.value, nq.value


@pytest.mark.parametrize("nb,m,tail_rows,max_q,ragged", [(1 << 15, 1, 64, 5, 0), ((1 << 14) + 7, 2, 32, 4, 1), (5000, 3, 16, 3, 0)])
def test_batched_solve_on_a_several_stage_plan(mg, ctx, oracle, monkeypatch, nb, m, tail_rows, max_q, ragged):
    """the plans of tests/test_gpu_coarse_cr.py::test_cr_several_stages (the boundary system of one chunk stage is the input
    of the next; the knobs shrink tail and chunks so that a small system takes such a plan), for a group of columns: every
    later stage reads and writes the K-column work space with its per-column strides.  ragged: one trailing row dropped, the
    group goes through the padded staging vectors.  K = 3, ld = N (in place where the system is not padded) and ld = N + 3
    (every other column off the 16 bytes: staged): every column bitwise the single-column solve, gap rows untouched"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A = block_tridiag(nb, m, seed=nb + m, ragged=ragged)
    N, K = A.shape[0], 3
    H, q, nq = _stage0_plan(mg, ctx, A)
    if ragged:
        # aggmg_coarse_plan reports the chunks of a system whose blocks are all complete (the partitioned phases take no
        # other); the plan itself depends on the block count, the block size and the knobs alone: ask the complete system
        assert q == -1
        Hfull, q, nq = _stage0_plan(mg, ctx, block_tridiag(nb, m, seed=nb + m))
        Hfull.free()
    assert 0 < q <= max_q and nq * m > tail_rows          # more than one stage
    info = H.coarse_info()
    assert info["on_device"] and info["block_size"] == m and (N + m - 1) // m == nb, info
    B = _rhs(oracle, N)[:, :K]
    z = ctx.to_device(np.zeros(N))
    ref = np.empty((N, K))
    for j in range(K):
        x = ctx.alloc(N)
        H.vcycle_dev(z, ctx.to_device(B[:, j]), x, 0, 0, 1.0)
        ref[:, j] = x.download()
    for ld in (N, N + 3):
        dB = _upload(ctx, B, ld)
        dX = ctx.to_device(np.full(ld * K, np.nan))
        H.coarse_solve_multi_dev(dB, dX, K, ld)
        got = dX.download().reshape((ld, K), order="F")
        for j in range(K):
            assert np.array_equal(got[:N, j], ref[:, j]), (ld - N, j, float(np.max(np.abs(got[:N, j] - ref[:, j]))))
        assert np.isnan(got[N:]).all()
    H.free()


# ---- through the public solvers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(mg, oracle):
    """65536 fine elements, ratios (4, 2, 2): the coarsest system has 4096 blocks of 2 -- one chunk stage + tail.  H1: the
    default context; H0: AGGMG_OPT_MG_CHECKPOINT = 0, the single-column form whose histories the K-column loop reproduces
    bit for bit (tests/test_gpu_multi_solve.py)"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    c1, c0 = mg.Context(0), mg.Context(0)
    c0.set_option(_lib.OPT_MG_CHECKPOINT, 0)
    U = UniformDgAggHierarchy(65536, p=3, pAgg=1, ratios=(4, 2, 2))
    H1, H0 = build_device_hierarchy(U, c1), build_device_hierarchy(U, c0)
    assert H1.multi_info(8) == (True, 8)
    info = H1.coarse_info()
    assert info["on_device"] and info["block_size"] == 2 and info["tail_blocks"] < 4096, info
    b = U.rhs()
    N, K = len(b), 8
    B = np.column_stack([b * (1.0 + j) if j % 2 == 0 else oracle.splitmix_normal(N, 40 + j) for j in range(K)])
    X0 = np.column_stack([oracle.splitmix_normal(N, 60 + j) for j in range(K)]) * (10.0 ** -np.arange(K))
    return dict(H1=H1, H0=H0, c1=c1, N=N, K=K, B=B, X0=X0, level=H1.nlevels - 1)


def test_v_cycle_on_matrices(mg, big):
    H, B, X0, K = big["H1"], big["B"], big["X0"], big["K"]
    X = mg.multigrid_v_cycle(H, X0, B)
    for j in range(K):
        xs = mg.multigrid_v_cycle(H, X0[:, j].copy(), B[:, j].copy())
        assert np.array_equal(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
    assert np.array_equal(mg.multigrid_v_cycle(H, X0, B), X)          # run to run


def test_pcg_on_matrices(mg, big):
    H, B, K = big["H1"], big["B"], big["K"]
    X, its, res = mg.pcg(H, B, maxiter=5, tol=1e-6)
    for j in range(K):
        xs, its0, res0 = mg.pcg(H, B[:, j].copy(), maxiter=5, tol=1e-6)
        assert int(its[j]) == its0 and res[j] == res0, j
        assert np.array_equal(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))


def test_multigrid_on_matrices_with_exact_solutions(mg, big):
    H1, H0, B, X0, N, K = big["H1"], big["H0"], big["B"], big["X0"], big["N"], big["K"]
    maxiter, tol = 4, 1e-3
    X, its, res, err = mg.multigrid(H1, X0, B, maxiter, tol, exact=True)
    assert all(len(e) == len(r) > 0 for e, r in zip(err, res))
    for j in range(K):
        xs, its0, res0, err0 = mg.multigrid(H0, X0[:, j].copy(), B[:, j].copy(), maxiter, tol, exact=True)
        assert int(its[j]) == its0 and res[j] == res0 and err[j] == err0, j
        assert np.array_equal(X[:, j], xs), (j, float(np.max(np.abs(X[:, j] - xs))))
    # the same call with the exact solutions supplied column by column
    c = big["c1"]
    ds = mg.DirectSolver(H1._ops[0])
    assert ds.where == "device"
    U = np.column_stack([ds.solve_dev(c.to_device(B[:, j].copy())).download() for j in range(K)])
    dX0, dB, dX, dU = (mg.DeviceMatrix(c, N, K) for _ in range(4))
    dX0.upload(X0)
    dB.upload(B)
    dU.upload(U)
    ncyc, res2, err2, _ = H1.multigrid_multi_dev(dX0, dB, dX, maxiter, tol, U_exact=dU)
    assert np.array_equal(ncyc, its) and res2 == res and err2 == err
    assert np.array_equal(dX.download(), X)


def test_one_coarse_launch_sequence_per_group(mg, big):
    H, c, N, level = big["H1"], big["c1"], big["N"], big["level"]
    for K, groups in ((8, 1), (9, 2)):
        dB, dX = mg.DeviceMatrix(c, N, K), mg.DeviceMatrix(c, N, K)
        dB.upload(np.column_stack([big["B"][:, j % 8] for j in range(K)]))
        H.vcycle_multi_dev(None, dB, dX)                  # (work space for the group: allocated outside the profiled call)
        c.synchronize()
        c.profile_enable(True)
        try:
            c.profile_collect()
            H.vcycle_multi_dev(None, dB, dX)
            prof = c.profile_collect()
        finally:
            c.profile_enable(False)
        assert prof[("coarse", level)][1] == groups, (K, prof)
        assert prof[("fused_down", 0)][1] == groups and prof[("fused_up", 0)][1] == groups


def test_argument_errors(mg, ctx, oracle):
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.api import ArgumentError, DimensionMismatch
    c = _case(mg, ctx, oracle, "scalar_1000")
    H, N, K = c["H"], c["N"], 3
    dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
    with pytest.raises(ArgumentError):
        H.coarse_solve_multi_dev(dB, dX, 0, N)               # ncols < 1
    with pytest.raises(ArgumentError):
        H.coarse_solve_multi_dev(dB, dX, K, N - 1)           # ld < N
    with pytest.raises(ArgumentError):
        H.coarse_solve_multi_dev(dB, dB)                     # X is B
    with pytest.raises(ArgumentError):
        H.coarse_solve_multi_dev(dB, None)                   # NULL X
    with pytest.raises(DimensionMismatch):
        H.coarse_solve_multi_dev(mg.DeviceMatrix(ctx, N + 1, K), dX)
    with pytest.raises(DimensionMismatch):
        H.coarse_solve_multi_dev(dB, mg.DeviceMatrix(ctx, N, K - 1))
    with pytest.raises(ArgumentError):
        H.coarse_solve_multi_dev(np.zeros((N, K)), dX)       # a host array for B
    ds = mg.DirectSolver(c["op"])
    with pytest.raises(ArgumentError):
        ds.solve_dev(np.zeros((N, K)))
    with pytest.raises(DimensionMismatch):
        ds.solve_dev(mg.DeviceMatrix(ctx, N + 1, K))
    # a hierarchy whose coarsest solve is the caller's
    Ho, _ = oracle.build_dg_agg_hierarchy(64, p=3, pAgg=1, nAgg=3, first=4)
    He = mg.MeshHierarchy.from_reference(Ho, ctx=ctx, coarse_mode=_lib.COARSE_EXTERNAL)
    Ne = He._ops[-1].shape[0]
    with pytest.raises(ArgumentError):
        He.coarse_solve_multi_dev(mg.DeviceMatrix(ctx, Ne, 2), mg.DeviceMatrix(ctx, Ne, 2))
    He.free()
