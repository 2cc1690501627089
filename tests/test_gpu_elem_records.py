"""The element-thread kernels with the class records in LDS (csrc/elem_kernels.hpp, btd_elem_rec_kernel /
btd_elem_rec_replay_up_kernel; AGGMG_OPT_ELEMENT_RECORDS_LDS): the level's table of packed class records is copied into
LDS at entry and every operator word read from there, pcol = B^{-1} q_{e-1} comes with the record instead of 16 FMAs per
element.  The same expressions otherwise, so every result must equal BIT FOR BIT both the element-thread kernels' with the
record words from global memory (option 0) and the plain kernels' (dictionary off), compared as 64-bit patterns.  Three
arms per case, each running vcycle_dev x 3 (the descent that stores nothing and the replaying ascent) and vcycles_dev(3)
(the storing descent, the launch between two cycles, the storing ascent); the first arm must have launched the new kernels
(aggmg_element_record_lds_launches), the other two must not.

What can go wrong is a wrong class record, record word, element, mask or rounding, so the shapes are the smallest that
put the level's first and last elements (their own classes), the tiles' ends (owned 248 / 250 / 240 / 244 of 256) and the
cap on classes everywhere.  Only powers of two have few classes (7); every other size of a few hundred elements has 40 or
more, over the cap of 32, so each case says whether it runs the new kernels (served=True, n = 256, 512, 1024 and n = 36
with 32 classes) or pins that a level over the cap keeps today's kernels and bits (served=False).  uniform.py has no
transfer whose first column is not unit at p = 3: only the records' unit form runs here (tests/test_elem_records_cpu.py packs both)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _ctx(mg, d, r, replay=1):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, d)
    if r is not None:
        ctx.set_option(_lib.OPT_ELEMENT_RECORDS_LDS, r)
    ctx.set_option(_lib.OPT_REPLAY_PRESMOOTH, replay)
    return ctx


@pytest.fixture(scope="module")
def arms(mg):
    """the three contexts: records in LDS (the default cap, not set) / records from global memory / the plain kernels"""
    return {"lds": _ctx(mg, 1, None), "global": _ctx(mg, 1, 0), "plain": _ctx(mg, 0, None)}


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(ctx, U, b, x0, ncyc, npre, npost, weights):
    """vcycle_dev x ncyc and vcycles_dev(ncyc) from x0 (None: no first iterate in the first cycle) ->
    (x, x of the loop, dictionary levels, launches with the records in LDS, element-thread launches, replayed cycles)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    H = build_device_hierarchy(U, ctx)
    if weights is not None:
        H.set_sweep_weights(0, weights[0], weights[1])
    N = len(b)
    bd = ctx.to_device(b)
    k0 = (ctx.element_record_lds_launches(), ctx.element_thread_launches(), ctx.replay_launches())
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
    k1 = (ctx.element_record_lds_launches(), ctx.element_thread_launches(), ctx.replay_launches())
    H.free()
    return (x, xl, levels) + tuple(a - b_ for a, b_ in zip(k1, k0))


CAP = 32   # the default of AGGMG_OPT_ELEMENT_RECORDS_LDS (test_option_values)


def _three(arms, U, b=None, x0=None, ncyc=3, npre=3, npost=3, weights=None, *, served):
    """served: must the new kernels have run (level 0 has no more classes than the cap), or must they not?"""
    b = U.rhs() if b is None else b
    xs, xls, lvs, ks, es, rs = _run(arms["lds"], U, b, x0, ncyc, npre, npost, weights)
    xg, xlg, lvg, kg, eg, rg = _run(arms["global"], U, b, x0, ncyc, npre, npost, weights)
    xp, xlp, lvp, kp, ep, rp = _run(arms["plain"], U, b, x0, ncyc, npre, npost, weights)
    assert lvp == {} and 0 in lvs and lvs == lvg, (lvs, lvg, lvp)
    assert (lvs[0] <= CAP) == served, f"level 0 has {lvs[0]} classes: the case is in the other arm"
    if served:
        assert ks > 0, "the kernels with the records in LDS did not run"
        assert ks == es, (ks, es)          # level 0 is the only level with blocks of 4 rows: every launch is served
    else:
        assert ks == 0
    assert kg == 0 and kp == 0, (kg, kp)
    assert es == eg and rs == rg, (es, eg, rs, rg)   # the same launches, the same replayed cycles
    assert np.all(np.isfinite(xp)) and np.any(xp != 0.0)
    for what, got, ref in (("lds / plain", xs, xp), ("global / plain", xg, xp), ("lds / plain, loop", xls, xlp),
                           ("global / plain, loop", xlg, xlp)):
        assert _same(got, ref), (what, float(np.max(np.abs(got - ref))))
    return lvs, ks, rs


def _hier(n, p=3, ratios=RATIOS, bc=None):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    return UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios, bc=bc)


def test_option_values(mg):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    cap, top = ctx.element_record_lds_cap()
    assert cap == top == 32
    ctx.set_option(_lib.OPT_ELEMENT_RECORDS_LDS, 7)
    assert ctx.element_record_lds_cap() == (7, 32)
    for bad in (-1, 33):
        with pytest.raises(mg.ArgumentError):
            ctx.set_option(_lib.OPT_ELEMENT_RECORDS_LDS, bad)
    assert ctx.element_record_lds_cap() == (7, 32)


@pytest.mark.parametrize("n", [256, 512])
def test_table_and_classes_bitwise(mg, arms, n):
    """a power-of-two mesh: 7 classes, the first and the last element in classes of their own"""
    lv, k, r = _three(arms, _hier(n), served=True)
    print(f"n={n}: classes per level {lv}, launches with the records in LDS {k}, replayed cycles {r}")
    assert lv[0] == 7 and r == 3


@pytest.mark.parametrize("n", [240, 256])
def test_boundary_arrangements_bitwise(mg, arms, n):
    """Dirichlet left / Neumann right: the first element's escape is on the other side.  n = 256 runs the new kernels;
    n = 240 has more classes than the cap and keeps today's"""
    served = n == 256
    _three(arms, _hier(n, bc=DIR_NEU), served=served)
    _three(arms, _hier(n, bc=DIR_NEU), x0=np.random.default_rng(n).standard_normal(4 * n), served=served)


def test_tens_of_classes_bitwise(mg, arms):
    """a mesh size that is no power of two: tens of classes, a table of more than one 16-byte word per thread"""
    lv, k, _ = _three(arms, _hier(MANY_N, ratios=MANY_RATIOS), served=True)
    print(f"n={MANY_N}: classes per level {lv}, launches with the records in LDS {k}")
    assert 12 < lv[0] <= 32   # (more than 256 / 21 classes: the second round of the table's loads)


def test_cap_at_and_below_the_class_count(mg):
    """the option set to the level's own class count serves the launches, one less does not; the same bits either way"""
    U = _hier(256)
    b = U.rhs()
    g = np.random.default_rng(7).standard_normal(len(b))
    out = {}
    for cap in (7, 6, 0):
        x, xl, lv, k, e, r = _run(_ctx(mg, 1, cap), U, b, g, 3, 3, 3, None)
        assert lv[0] == 7 and e > 0 and r == 3
        out[cap] = (x, xl, k, e)
    assert out[7][2] == out[7][3] and out[6][2] == 0 and out[0][2] == 0
    for cap in (7, 6):
        assert _same(out[cap][0], out[0][0]) and _same(out[cap][1], out[0][1])


def test_over_any_cap_bitwise(mg, arms):
    """n = 4608: 208 classes on level 0, more than the option takes: today's kernels, counter 0"""
    lv, k, _ = _three(arms, _hier(4096 + 512), served=False)
    assert lv[0] > 32 and k == 0


@pytest.mark.parametrize("n", [256, 512, 1024])
def test_tile_ends_with_the_table_bitwise(mg, arms, n):
    """The tiles' ends on the NEW kernels.  Only powers of two have few classes (7), so the owned ranges end where they
    end at those sizes: at n = 256 the second tile owns 8 elements of the descent (owned 248), 12 of the replaying ascent
    (244), 16 of the launch between two cycles (240) and 6 of the storing ascent (250), its right halo wholly outside the
    level; at 512 and 1024 there are three to five tiles, the last one short.  A random first iterate, and none."""
    U = _hier(n)
    lv, k, r = _three(arms, U, x0=np.random.default_rng(n).standard_normal(4 * n), served=True)
    assert lv[0] <= CAP and k > 0 and r == 3
    lv, k, r = _three(arms, U, served=True)
    assert lv[0] <= CAP and k > 0 and r == 3


@pytest.mark.parametrize("n", [248, 252, 496, 500, 240, 244, 250])
def test_tile_end_sizes_over_the_cap_bitwise(mg, arms, n):
    """The sizes at which an owned range ends exactly (248 descent, 240 between two cycles, 250 ascent, 244 replaying
    ascent; the multiple itself and one agglomerate past it; n = 250 in agglomerates of 2) all have 40 to 120 classes on
    level 0, MORE than the cap: these cases do NOT run the new kernels.  They pin that such a level keeps today's kernels
    (counter 0) and today's bits with the option on; the new kernels' tile ends are the test above."""
    lv, k, _ = _three(arms, _hier(n, ratios=RATIOS if n % 16 == 0 else (4,) if n % 4 == 0 else (2,)), served=False)
    assert lv[0] > CAP and k == 0


def test_exact_data_bitwise(mg, arms):
    """right-hand side and first iterate of exact small integers on the NEW kernels (n = 512: 7 classes, three tiles): a
    wrong record word (the precomputed pcol among them), element or row is a difference of order one; a random first
    iterate, and none"""
    U = _hier(512)
    N = len(U.rhs())
    rng = np.random.default_rng(5)
    b = rng.integers(-8, 9, N).astype(np.float64)
    g = rng.integers(-4, 5, N).astype(np.float64)
    for kw in (dict(b=b, x0=g), dict(b=b), dict(x0=np.random.default_rng(11).standard_normal(N)), dict(x0=None)):
        lv, k, _ = _three(arms, U, served=True, **kw)
        assert lv[0] <= CAP and k > 0


@pytest.mark.parametrize("ratios,n,served", [((2, 2, 2, 2), 496, False), ((2, 2, 2, 2), 512, True), ((8, 2, 2), 480, False),
                                             ((8, 2, 2), 512, True), ((4, 4, 4), 448, False), ((4, 4, 4), 512, True)])
def test_other_fine_ratios_bitwise(mg, arms, ratios, n, served):
    """agglomerates of 2 and 8 elements (and 4 all the way down): the prolongation's coarse index and the restriction's
    sums (through LDS at every ratio: the kernels carry no sum from lane to lane).  n = 512 runs the new kernels; 496,
    480 and 448 have more classes than the cap and keep today's -- each case says which"""
    lv, k, _ = _three(arms, _hier(n, ratios=ratios), x0=np.random.default_rng(n).standard_normal(4 * n), served=served)
    assert (lv[0] <= CAP) == served and (k > 0) == served, (lv, k)


@pytest.mark.parametrize("npre,npost", [(1, 1), (2, 3), (3, 0), (0, 3)])
def test_sweep_counts_bitwise(mg, arms, npre, npost):
    """other halos -- and launches without sweeps, which stay on the row-thread kernel beside the new ones (the cycle
    does not replay then: the storing descent / ascent)"""
    _, _, r = _three(arms, _hier(512), npre=npre, npost=npost, served=True)
    assert r == (3 if npre and npost else 0)


def test_sweep_weight_schedule_bitwise(mg, arms):
    """every sweep of a launch has its own weight (wts.w[sw]); the replaying launch takes w_pre ++ w_post"""
    g = np.random.default_rng(3).standard_normal(4 * 512)
    _three(arms, _hier(512), x0=g, weights=(np.array([0.9, 0.5, 0.7]), np.array([0.3, 0.8, 0.6])), served=True)


@pytest.mark.parametrize("replay", [1, 0])
def test_replayed_and_storing_cycles_bitwise(mg, replay):
    """the replayed cycle and the storing one (AGGMG_OPT_REPLAY_PRESMOOTH 1 / 0), each with the records in LDS and
    from global memory; a cycle of more sweeps than one launch has weights falls back to the storing launches"""
    U = _hier(1024)
    b = U.rhs()
    g = np.random.default_rng(23).standard_normal(len(b))
    for npre, npost, replays in ((3, 3, 3 * replay), (5, 4, 0)):
        xs, xls, _, ks, es, rs = _run(_ctx(mg, 1, None, replay), U, b, g, 3, npre, npost, None)
        xg, xlg, _, kg, eg, rg = _run(_ctx(mg, 1, 0, replay), U, b, g, 3, npre, npost, None)
        assert rs == rg == replays, (rs, rg, replays)
        assert ks == es == eg and ks > 0 and kg == 0, (ks, es, eg, kg)
        assert _same(xs, xg) and _same(xls, xlg)


def test_symmetric_residual_off_keeps_the_full_rows(mg):
    """without the symmetric residual form the record has no residual words: the launches that form a residual keep
    their kernel, the others are served; the same bits"""
    from agglomerationmultigrid1d_amd import _lib
    U = _hier(512)
    b = U.rhs()
    g = np.random.default_rng(31).standard_normal(len(b))
    out = []
    for r in (None, 0):
        ctx = _ctx(mg, 1, r)
        ctx.set_option(_lib.OPT_SYMMETRIC_RESIDUAL, 0)
        out.append(_run(ctx, U, b, g, 3, 3, 3, None))
    (xs, xls, _, ks, es, _), (xg, xlg, _, kg, eg, _) = out
    assert 0 < ks < es and es == eg and kg == 0, (ks, es, eg, kg)
    assert _same(xs, xg) and _same(xls, xlg)


MANY_N, MANY_RATIOS = 36, (4,)   # 32 classes: every element but a few is a class of its own
