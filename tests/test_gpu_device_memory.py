"""Device memory the library owns (csrc/devmem.hpp, C ABI aggmg_debug_device_memory): every handle gives back what it
took, nothing accumulates under a live context, and a set-up that refuses its input releases what it had allocated by
then.  The counters are the process's live allocations and bytes of the library's own arrays; DeviceVector /
DeviceMatrix storage belongs to the caller and is not counted.

The workload: a DG hierarchy (256 elements, p = 1, ratios (2, 2), block Jacobi: fused, paired and dictionary levels) and
a CG chain hierarchy (100 elements, p = 4 -> 2 -> 1 -> DG p = 0, point Jacobi: chain and chain-dictionary levels, cyclic
reduction at the coarsest); on each one V-cycle, multigrid (3 cycles, exact=True) and pcg (3 iterations), then K-column
cycles with K = 3, 5, 2 (the workspaces grow once, then stay); a Galerkin product and a BlockDiagonal LU."""
import gc

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def meshes():
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, UniformDgAggHierarchy
    return UniformDgAggHierarchy(256, p=1, ratios=(2, 2)), UniformCgDgHierarchy(100, ps=(4, 2, 1))


def live():
    from agglomerationmultigrid1d_amd.api import device_memory
    gc.collect()
    return device_memory()


def free_hierarchy(H):
    ds = H.__dict__.pop("_direct_solver", None)   # multigrid(exact=True) keeps the fine-level direct solver with H
    if ds is not None and ds.H is not None:
        ds.H.free()
    H.free()
    for obj in list(H.mSmoothers) + H._ops + H._Ls:
        obj.free()


def workload(mg, ctx, meshes):
    from agglomerationmultigrid1d_amd.uniform import build_device_cg_hierarchy, build_device_hierarchy
    Udg, Ucg = meshes
    Hdg = build_device_hierarchy(Udg, ctx)
    Hcg = build_device_cg_hierarchy(Ucg, ctx)
    assert Hdg.level_kinds()[:-1] == ["fused_btd"] * 2 and Hdg.dictionary_levels(), (Hdg.level_kinds(), Hdg.dictionary_levels())
    assert Hcg.level_kinds()[:-1] == ["fused_chain"] * 3 and Hcg.dictionary_levels(), (Hcg.level_kinds(), Hcg.dictionary_levels())
    assert Hcg.coarse_info()["on_device"]
    rng = np.random.default_rng(5)
    for H, U in ((Hdg, Udg), (Hcg, Ucg)):
        b = U.rhs()
        z = np.zeros(len(b))
        mg.multigrid_v_cycle(H, z, b)
        mg.multigrid(H, z, b, 3, 0.0, exact=True)
        mg.pcg(H, b, maxiter=3, tol=0.0)
        for K in (3, 5, 2):
            B = np.asfortranarray(rng.standard_normal((len(b), K)))
            X = mg.multigrid_v_cycle(H, np.zeros_like(B), B)
            assert X.shape == B.shape and np.all(np.isfinite(X))
    # a Galerkin product A * L, and a block-diagonal LU of 3 blocks of size 2
    AL = Hdg._ops[0].matmul(Hdg._Ls[0])
    assert AL.shape == (Hdg._ops[0].shape[0], Hdg._Ls[0].shape[1])
    AL.free()
    lu = mg.BlockDiagonal([np.array([[2.0, 1.0], [1.0, 3.0]]) + k * np.eye(2) for k in range(3)], ctx).lu()
    assert np.allclose(lu.solve(np.ones(6))[:2], np.linalg.solve([[2.0, 1.0], [1.0, 3.0]], np.ones(2)))
    lu._dev.free()
    free_hierarchy(Hdg)
    free_hierarchy(Hcg)


def test_everything_comes_back(mg, meshes):
    before = live()
    ctx = mg.Context(0)
    workload(mg, ctx, meshes)
    ctx.close()
    assert live() == before


def test_nothing_accumulates_under_a_live_context(mg, meshes):
    ctx = mg.Context(0)
    after = []
    for _ in range(3):
        workload(mg, ctx, meshes)
        after.append(live())
    ctx.close()
    # (the context's grow-only work space has reached its size after the first round)
    assert after[1] == after[2], after


def refused(exc, fn):
    """fn raises exc and leaves the counters where they were.  It runs once before the measured call: a set-up may be the
    first to ask for one of the context's grow-only buffers (the probe solve of aggmg_hier_create takes norms), which
    stay with the context by design."""
    with pytest.raises(exc):
        fn()
    before = live()
    with pytest.raises(exc):
        fn()
    assert live() == before


def test_refused_setups_release_what_they_took(mg, meshes):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    Udg, _ = meshes
    # a singular block in the middle of a block-diagonal factorisation: AGGMG_ERR_SINGULAR from aggmg_blockdiag_setup
    refused(mg.SingularException, lambda: mg.BlockDiagonal([np.eye(2), np.zeros((2, 2)), np.eye(2)], ctx).lu())
    # red-black block Gauss-Seidel on index lists that are not contiguous: AGGMG_ERR_UNSUPPORTED from aggmg_blockjacobi_setup
    A = mg.DeviceOperator(Udg.stiffness_csc(0), _lib.OP_STIFFNESS, ctx)
    inds = np.asarray(Udg.descriptor(0).mBlockInds, dtype=np.int64)
    m, nb = inds.shape
    strided = (np.arange(m)[:, None] * nb + np.arange(nb)[None, :] + 1).astype(np.int64)   # block k = {k, k + nb, ...}
    assert sorted(strided.ravel()) == sorted(inds.ravel())
    refused(mg.UnsupportedError, lambda: mg.BlockGaussSeidel(A, strided, ctx))
    A.free()
    # device cyclic reduction forced on a coarsest operator its probe solve rejects (tests/test_gpu_coarse_cr.py:
    # tridiagonal with a diagonal of 1e-9, element growth 1 / eps): AGGMG_ERR_UNSUPPORTED from aggmg_hier_create
    n = 4096 + 512
    T = mg.DeviceOperator(sp.diags([np.ones(n - 1), np.full(n, 1e-9), np.ones(n - 1)], [-1, 0, 1], format="csc"),
                          _lib.OP_STIFFNESS, ctx)
    refused(mg.UnsupportedError,
            lambda: mg.MeshHierarchy(None, [T], [], [], ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_DEVICE_CR))
    T.free()
    ctx.close()
