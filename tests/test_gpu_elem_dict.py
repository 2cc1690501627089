"""Element-thread kernel of the dictionary launches (csrc/elem_kernels.hpp, btd_elem_dict_kernel; AGGMG_OPT_ELEMENT_THREADS):
one thread owns an element of a p = 3 level -- its four rows in registers, tiles of 256 elements in one slab -- where the
row-thread dictionary variant of btd_fused_kernel gives every row a thread.  It repeats that kernel's expressions, so
every result must equal BIT FOR BIT both the row-thread dictionary kernel's (option off) and the plain kernel's
(dictionary off), compared as 64-bit patterns.  Three arms per case, each running vcycle_dev x 3 and vcycles_dev(3)
(descent, ascent and the launch between two cycles); the first arm must have launched the element-thread kernel
(aggmg_element_thread_launches), the other two must not.

What can go wrong is a wrong element, row, mask or rounding at a tile's or the level's end, so the shapes are the smallest
that put those ends everywhere: the planner's owned ranges for 256-element tiles -- 248 (descent: 3 sweeps + the residual's
row, halo 4), 250 (ascent: halo 3) and 240 (between two cycles: 6 sweeps + 1, halo 7, whole agglomerates of 4) -- with n
at, one agglomerate past and on either side of their multiples."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)
TILE = 256                                  # elements of an element-thread tile (kElemThreads)


def _owned(halo, align):
    """host_plan.hpp fused_tile_plan(te = 256, halo, align) for equal agglomerates: te - 2 halo rounded down to whole ones"""
    return ((TILE - 2 * halo) // align) * align


def _tile_ns(rho=4, npre=3, npost=3):
    """n at the ends of the three launches' owned ranges -> sorted list of (n, ratios); the ratios are (4, 2, 2) where
    they divide n and (4,) -- two levels -- where only the fine ratio does"""
    owned = {"descent": _owned(npre + 1, rho), "ascent": _owned(npost, 1), "between": _owned(npre + npost + 1, rho)}
    ns = set()
    for o in owned.values():
        for k in (1, 2, 3):
            m = k * o
            m4 = -(-m // rho) * rho
            ns.update((m4, m4 + rho))                  # the multiple itself / a last tile owning one agglomerate
            ns.update(((m // 16) * 16, (m // 16 + 1) * 16))   # either side, with all three ratios
    ns = sorted(n for n in ns if n <= 3 * 248 + 16)
    return owned, [(n, RATIOS if n % 16 == 0 else (rho,)) for n in ns]


OWNED, TILE_NS = _tile_ns()


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def arms(mg):
    """the three contexts: element threads / row threads (both with the dictionary) / the plain kernel"""
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    for name, d, e in (("elem", 1, 1), ("row", 1, 0), ("plain", 0, 1)):
        ctx = mg.Context(0)
        ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, d)
        ctx.set_option(_lib.OPT_ELEMENT_THREADS, e)
        out[name] = ctx
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(ctx, U, b, x0, ncyc, npre, npost, weights):
    """vcycle_dev x ncyc and vcycles_dev(ncyc) from x0 (None: no first iterate in the first cycle) ->
    (x, x of the loop, dictionary levels, element-thread launches)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    H = build_device_hierarchy(U, ctx)
    if weights is not None:
        H.set_sweep_weights(0, weights[0], weights[1])
    N = len(b)
    bd = ctx.to_device(b)
    before = ctx.element_thread_launches()
    xa, xb = ctx.alloc(N), ctx.alloc(N)
    src = None if x0 is None else ctx.to_device(x0)
    for _ in range(ncyc):
        H.vcycle_dev(src, bd, xb, npre, npost)
        xa, xb = xb, xa
        src = xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N) if x0 is None else x0), bd, xb, ncyc, npre, npost)
    xl = xb.download()
    levels = H.dictionary_levels()
    launches = ctx.element_thread_launches() - before
    H.free()
    return x, xl, levels, launches


def _three(arms, U, b=None, x0=None, ncyc=3, npre=3, npost=3, weights=None):
    b = U.rhs() if b is None else b
    xe, xle, lve, ke = _run(arms["elem"], U, b, x0, ncyc, npre, npost, weights)
    xr, xlr, lvr, kr = _run(arms["row"], U, b, x0, ncyc, npre, npost, weights)
    xp, xlp, lvp, kp = _run(arms["plain"], U, b, x0, ncyc, npre, npost, weights)
    assert lvp == {} and 0 in lve and lve == lvr, (lve, lvr, lvp)
    assert ke > 0, "the element-thread kernel did not run"
    assert kr == 0 and kp == 0, (kr, kp)
    assert np.all(np.isfinite(xp)) and np.any(xp != 0.0)
    for what, got, ref in (("elem / plain", xe, xp), ("row / plain", xr, xp), ("elem / plain, loop", xle, xlp),
                           ("row / plain, loop", xlr, xlp)):
        assert _same(got, ref), (what, float(np.max(np.abs(got - ref))))
    assert _same(xle, xe)   # (no first iterate and a zero one are the same cycle)
    return lve, ke


def _hier(n, p=3, ratios=RATIOS, bc=None):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    return UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios, bc=bc)


def test_planner_owned_ranges():
    """the owned ranges the shapes below are derived from"""
    print(f"owned per 256-element tile: {OWNED}; n: {[n for n, _ in TILE_NS]}")
    assert OWNED == {"descent": 248, "ascent": 250, "between": 240}


@pytest.mark.parametrize("n,ratios", TILE_NS)
def test_tile_edges_bitwise(mg, arms, n, ratios):
    """one tile exactly, a last tile owning one agglomerate, a last tile whose right halo lies wholly outside the level,
    n on both sides of the multiples of 248 / 250 / 240"""
    lv, k = _three(arms, _hier(n, ratios=ratios))
    print(f"n={n} ratios={ratios}: classes per level {lv}, element-thread launches {k}")


@pytest.mark.parametrize("n", [112, 128, 224, 240, 256, 272, 352])
def test_row_thread_tile_edges_bitwise(mg, arms, n):
    """the row-thread variant's own edges (two slabs of 64 elements, owned 120 / 112: tests/test_gpu_dict_tiles.py), now
    that it is no longer the default -- and the level's ends inside an element-thread tile"""
    _three(arms, _hier(n))


@pytest.mark.parametrize("n", [240, 256])
def test_boundary_arrangements_bitwise(mg, arms, n):
    """Dirichlet left / Neumann right: the first and last elements' records change places (the escape at e = 0)"""
    _three(arms, _hier(n, bc=DIR_NEU))


def test_initial_guess_bitwise(mg, arms):
    """a non-zero random first iterate (the u_in stream), and none (its load dropped)"""
    U = _hier(496)
    g = np.random.default_rng(11).standard_normal(len(U.rhs()))
    _three(arms, U, x0=g)
    _three(arms, U, x0=None)


def test_exact_data_bitwise(mg, arms):
    """right-hand side and first iterate of exact small integers: a wrong element or row is a difference of order one"""
    U = _hier(496)
    N = len(U.rhs())
    rng = np.random.default_rng(5)
    b = rng.integers(-8, 9, N).astype(np.float64)
    g = rng.integers(-4, 5, N).astype(np.float64)
    _three(arms, U, b=b, x0=g)
    _three(arms, U, b=b)


@pytest.mark.parametrize("ratios,n", [((2, 2, 2, 2), 496), ((2, 2, 2, 2), 512), ((8, 2, 2), 480), ((8, 2, 2), 512),
                                      ((4, 4, 4), 448), ((4, 4, 4), 512)])
def test_other_fine_ratios_bitwise(mg, arms, ratios, n):
    """agglomerates of 2 and 8 elements (and 4 all the way down): the prolongation's coarse index and the restriction's
    sums against a 4-element habit"""
    rho = ratios[0]
    print(f"ratios={ratios}: owned {_owned(4, rho)} / {_owned(3, 1)} / {_owned(7, rho)}")
    _three(arms, _hier(n, ratios=ratios))


@pytest.mark.parametrize("npre,npost", [(1, 1), (2, 3), (3, 0), (0, 3)])
def test_sweep_counts_bitwise(mg, arms, npre, npost):
    """other halos -- and launches without sweeps, which stay on the row-thread kernel beside element-thread ones"""
    _three(arms, _hier(512), npre=npre, npost=npost)


def test_sweep_weight_schedule_bitwise(mg, arms):
    """a Chebyshev schedule on the fine level: every sweep of a launch has its own weight (wts.w[sw])"""
    w = mg.chebyshev_weights(1.9, degree=3)
    assert len(set(np.asarray(w).tolist())) == 3
    _three(arms, _hier(512), weights=(w, w[::-1].copy()))
    g = np.random.default_rng(3).standard_normal(4 * 512)
    _three(arms, _hier(512), x0=g, weights=(np.array([0.9, 0.5, 0.7]), np.array([0.3, 0.8, 0.6])))


def test_many_classes_bitwise(mg, arms):
    """a mesh size that is no power of two: more distinct records than a power-of-two mesh gives"""
    lv, k = _three(arms, _hier(4096 + 512))
    print(f"n={4096 + 512}: classes per level {lv}, element-thread launches {k}")
    assert lv[0] >= 3
