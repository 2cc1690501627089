"""Tiles of the dictionary variant of the fused fine-level kernel (csrc/kernels.hpp, btd_fused_kernel<..., DICT = true>):
its load phase reads cls, b, u_in and the coarse pair of every slab straight-line -- a lane outside the level reads
the nearest element inside it and is masked afterwards -- and its residual decodes the record words of all slabs at once, with the escapes
(the level's first element) patched in a second pass.  What can go wrong is a wrong element, row or mask at a tile's or
the level's end, so the shapes are the smallest that put those ends everywhere: one tile exactly, a last tile with a few
owned elements, a last tile whose second slab lies wholly outside the level, owned ranges of 120 (a cycle's descent and
ascent) and 112 (the launch between two cycles: 6 sweeps and a residual, halo 7) on either side of a multiple.

Oracle: the same cycles with the option off -- the plain kernel, which this change leaves alone -- compared as 64-bit
patterns (the dictionary's loads return the operator's own bits from another address)."""
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


def _uniform(U, b=None):
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    return lambda ctx: (build_device_hierarchy(U, ctx), U.rhs() if b is None else b)


def _on_off(mg, build, x0=None):
    x1, xl1, lv1 = _run(mg, build, True, x0)
    x0_, xl0, lv0 = _run(mg, build, False, x0)
    assert lv0 == {}, lv0
    assert 0 in lv1, lv1   # the fine level took the dictionary: the variant under test ran
    assert np.all(np.isfinite(x0_)) and np.any(x0_ != 0.0)
    assert _same(x1, x0_), float(np.max(np.abs(x1 - x0_)))
    assert _same(xl1, xl0), float(np.max(np.abs(xl1 - xl0)))
    assert _same(xl1, x1)
    return lv1


def _hier(n, p, bc=None):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    return UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=RATIOS, bc=bc)


@pytest.mark.parametrize("n", [112, 128, 224, 240, 256, 272, 352])
def test_tile_edges_bitwise(mg, n):
    """p = 3 (blocks of 4 rows, two slabs of 64 elements): the level's two ends in every position of a tile"""
    lv = _on_off(mg, _uniform(_hier(n, 3)))
    print(f"n={n}: classes per level {lv}")


@pytest.mark.parametrize("n", [112, 240])
def test_boundary_arrangements_bitwise(mg, n):
    """Dirichlet left / Neumann right: the first and last elements' records change places"""
    _on_off(mg, _uniform(_hier(n, 3, bc=DIR_NEU)))


@pytest.mark.parametrize("n", [240, 256, 496, 512])
def test_block_size_two_bitwise(mg, n):
    """p = 1 (blocks of 2 rows, one slab of 128 elements)"""
    _on_off(mg, _uniform(_hier(n, 1)))


def test_initial_guess_bitwise(mg):
    """a non-zero random first iterate (the u_in stream) and the zero one given as no iterate at all (its load dropped)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    U = _hier(240, 3)
    b = U.rhs()
    g = np.random.default_rng(11).standard_normal(len(b))
    _on_off(mg, _uniform(U), x0=g)
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        assert (0 in H.dictionary_levels()) == on
        bd, xd = ctx.to_device(b), ctx.alloc(len(b))
        H.vcycle_dev(None, bd, xd)   # x0 = None: the fine level reads no iterate
        out.append(xd.download())
        H.free()
    assert np.any(out[1] != 0.0)
    assert _same(out[0], out[1])


def test_exact_data_bitwise(mg):
    """right-hand side and first iterate of exact small integers: a wrong element or row is a difference of order one,
    not one in the last place"""
    U = _hier(240, 3)
    N = len(U.rhs())
    rng = np.random.default_rng(5)
    b = rng.integers(-8, 9, N).astype(np.float64)
    g = rng.integers(-4, 5, N).astype(np.float64)
    _on_off(mg, _uniform(U, b), x0=g)
    _on_off(mg, _uniform(U, b))
