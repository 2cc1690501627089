"""Operator dictionary (AGGMG_OPT_OPERATOR_DICTIONARY; csrc/kernels.hpp btd_fused_kernel<..., DICT = true>, set-up
csrc/setup.hip setup_op_dictionary): on a uniform mesh the per-element operator records repeat, the level keeps one
copy of every distinct record and the block-Jacobi launches of a cycle index the operator by the element's class.  The
loads return the operator's own bits from another address, so every result must equal the run with the option off BIT
FOR BIT (compared as 64-bit patterns: stricter than ==, and indifferent to what the values are).  The tests switch the
option on and off explicitly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _ctx(mg, on):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
    return ctx


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(mg, build, on, x0=None, ncyc=3):
    """vcycle_dev x ncyc and vcycles_dev(ncyc) from x0 (None: the zero guess) -> (x, x of the loop, dictionary levels)"""
    ctx = _ctx(mg, on)
    H, b = build(ctx)
    N = len(b)
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(np.zeros(N) if x0 is None else x0), ctx.alloc(N)
    for _ in range(ncyc):
        H.vcycle_dev(xa, bd, xb)
        xa, xb = xb, xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N) if x0 is None else x0), bd, xb, ncyc)
    xl = xb.download()
    levels = H.dictionary_levels()
    H.free()
    return x, xl, levels


def _uniform(U, smoother="blockJac"):
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    return lambda ctx: (build_device_hierarchy(U, ctx, smoother=smoother), U.rhs())


def _on_off(mg, build, x0=None):
    x1, xl1, lv1 = _run(mg, build, True, x0)
    x0_, xl0, lv0 = _run(mg, build, False, x0)
    assert lv0 == {}, lv0
    assert _same(x1, x0_), float(np.max(np.abs(x1 - x0_)))
    assert _same(xl1, xl0) and _same(xl1, x1)
    return lv1


def _cpu_classes(U):
    """distinct per-element INPUT records of the fine level (sub, diagonal, super block, rows of L): every one of them
    is stored whole in the device record, so the device has at least as many classes"""
    sub, diag, sup = U.levels[0]["A"]
    ne = diag.shape[0]
    rec = np.concatenate([np.asarray(x).reshape(ne, -1) for x in (sub, diag, sup, U.transfers[0]["Lb"])], axis=1)
    return len(np.unique(np.ascontiguousarray(rec).view(np.uint64), axis=0))


@pytest.mark.parametrize("bc", [None, DIR_NEU], ids=["neu-dir", "dir-neu"])
@pytest.mark.parametrize("n", [16, 48, 256, 4096, 3072])
def test_config34_cycles_bitwise(mg, n, bc):
    """the benchmark's hierarchy: levels smaller than a tile and tiles cut by both domain ends (16, 48, 256), a handful
    of classes (4096), a non-dyadic n with on the order of a hundred (3072); both boundary arrangements -- the first
    element's coupling takes the escape, so the dictionary's scol / dblk copies are read"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=RATIOS, bc=bc)
    lv = _on_off(mg, _uniform(U))
    print(f"n={n} bc={'default' if bc is None else 'dir/neu'}: classes per level {lv}, CPU input classes {_cpu_classes(U)}")
    assert 0 in lv and 1 <= lv[0] <= min(n, 1024), lv
    if n == 4096:
        assert lv[0] <= 16, lv


def test_nonzero_guess_and_halves_bitwise(mg):
    """a non-zero first guess, the zero guess given as x0 = None, and the two halves of the cycle called on their own
    (descent: sweeps, residual, restriction; ascent: prolongation, sweeps), the coarsest right-hand side compared"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(4096, p=3, pAgg=1, ratios=RATIOS)
    b = U.rhs()
    g = np.random.default_rng(7).standard_normal(len(b))
    assert 0 in _on_off(mg, _uniform(U), x0=g)
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        bd, xd = ctx.to_device(b), ctx.alloc(len(b))
        res = []
        for guess in (g, np.zeros(len(b))):
            H.vcycle_down_dev(ctx.to_device(guess), bd)
            rhs_ptr, sol_ptr, nc = H.coarse_buffers()
            rc = np.empty(nc)
            ctx.synchronize()
            ctx.check(ctx.lib.aggmg_memcpy_d2h(ctx.handle, rc.ctypes.data, rhs_ptr, nc * 8))
            res.append(rc)
        H.vcycle_dev(None, bd, xd)               # x0 = None: the zero guess, the fine level reads no iterate
        res.append(xd.download())
        H.vcycle_dev(ctx.to_device(g), bd, xd)   # (leaves a coarsest solution for the ascent alone)
        H.vcycle_up_dev(bd, xd)
        res.append(xd.download())
        out.append(res)
        H.free()
    for r1, r0 in zip(*out):
        assert _same(r1, r0)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_polynomial_degrees_bitwise(mg, p):
    """blocks of 2 and 4 rows (p = 1, 3) may take the form, the others must not; the same bits either way"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(2**12, p=p, pAgg=1, ratios=RATIOS)
    lv = _on_off(mg, _uniform(U))
    print(f"p={p}: classes per level {lv}")
    if p in (2, 4):
        assert 0 not in lv, lv
    if p == 3:
        assert 0 in lv, lv


def test_ragged_hierarchy_keeps_the_full_arrays(mg):
    """perturbed fine mesh, agglomerates of different sizes: no dictionary on the fine level"""
    from agglomerationmultigrid1d_amd.uniform import build_device_ragged_hierarchy

    def build(ctx):
        H, b, _ = build_device_ragged_hierarchy(2**10, ctx)
        return H, b
    lv = _on_off(mg, build)
    assert 0 not in lv, lv


def test_too_many_classes_keeps_the_full_arrays(mg):
    """a uniform mesh of an interval whose vertices round in many different ways: more distinct records than the
    dictionary takes (counted on the CPU first), so the fine level keeps the plain path"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(160000, p=3, pAgg=1, ratios=RATIOS, xin=-1.0 / 3.0, xout=1.0e9 + 0.7)
    ncpu = _cpu_classes(U)
    print(f"CPU input classes {ncpu}")
    assert ncpu > 1024
    lv = _on_off(mg, _uniform(U))
    assert 0 not in lv, lv


def test_multigrid_with_checkpoints_bitwise(mg):
    """the device-resident loop with the checkpoint on: its launches keep the full arrays; histories compared too"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(2**12, p=3, pAgg=1, ratios=RATIOS)
    b = U.rhs()
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        ctx.set_option(_lib.OPT_MG_CHECKPOINT, 1)
        H = build_device_hierarchy(U, ctx)
        assert (0 in H.dictionary_levels()) == on
        res = []
        for every in (1, 3):
            x, it, r = mg.multigrid_dev(H, ctx.to_device(np.zeros(len(b))), ctx.to_device(b), 9, 1e-30, check_every=every)
            res.append((x.download(), it, list(r)))
        out.append(res)
        H.free()
    for (x1, it1, r1), (x0, it0, r0) in zip(*out):
        assert it1 == it0 and r1 == r0
        assert _same(x1, x0)


def test_block_gauss_seidel_bitwise(mg):
    """red-black block Gauss-Seidel levels: the dictionary is built, the Gauss-Seidel variant reads the full arrays"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(2**12, p=3, pAgg=1, ratios=RATIOS)
    _on_off(mg, _uniform(U, smoother="blockGS"))


def test_multi_column_cycle_bitwise(mg):
    """one K-column cycle: its kernels keep the full arrays; every column is also the single-column cycle's bits"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(2**12, p=3, pAgg=1, ratios=RATIOS)
    N, K = len(U.rhs()), 3
    B = np.random.default_rng(3).standard_normal((N, K))
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
        dB.upload(B)
        H.vcycle_multi_dev(None, dB, dX)
        X = dX.download()
        xd = ctx.alloc(N)
        H.vcycle_dev(ctx.to_device(np.zeros(N)), ctx.to_device(np.ascontiguousarray(B[:, 1])), xd)
        out.append((X, xd.download()))
        H.free()
    (X1, c1), (X0, c0) = out
    assert _same(X1, X0) and _same(c1, c0)
    assert _same(np.ascontiguousarray(X1[:, 1]), c1)
