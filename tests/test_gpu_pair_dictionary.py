"""Operator dictionary of the two-level launches (csrc/pair_kernels.hpp btd_pair_down_dict_kernel /
btd_pair_up_dict_kernel, set-up csrc/setup.hip setup_pair_dictionary): the dense m = 2 levels a paired launch takes keep
one copy of every distinct per-element operator record, and the launch indexes the operator by the element's class when
BOTH of its levels have a dictionary.  The loads return the operator's own bits from another address and the arithmetic
is the plain kernels', so every result must equal the run with AGGMG_OPT_OPERATOR_DICTIONARY off BIT FOR BIT (compared
as 64-bit patterns).  The tests switch the options explicitly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _ctx(mg, on, pair=True):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
    ctx.set_option(_lib.OPT_PAIR_LEVELS, 1 if pair else 0)
    return ctx


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _cpu_classes(U, k):
    """distinct per-element INPUT records of level k (sub, diagonal, super block, rows of L): every one of them is stored
    whole in the device record, so the device has at least as many classes"""
    sub, diag, sup = U.levels[k]["A"]
    ne = diag.shape[0]
    rec = np.concatenate([np.asarray(x).reshape(ne, -1) for x in (sub, diag, sup, U.transfers[k]["Lb"])], axis=1)
    return len(np.unique(np.ascontiguousarray(rec).view(np.uint64), axis=0))


def _run(mg, U, on, sweeps=(3, 3), pair=True, x0=None, ncyc=3, weights=None):
    """vcycle_dev x ncyc and vcycles_dev(ncyc) -> (x, x of the loop, dictionary levels, levels whose descent / ascent at
    these sweep counts carries the next level too)"""
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    nPre, nPost = sweeps
    ctx = _ctx(mg, on, pair)
    H = build_device_hierarchy(U, ctx)
    if weights:
        for k, (pre, post) in weights.items():
            H.set_sweep_weights(k, pre, post)
    b = U.rhs()
    N = len(b)
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(np.zeros(N) if x0 is None else x0), ctx.alloc(N)
    for _ in range(ncyc):
        H.vcycle_dev(xa, bd, xb, nPre=nPre, nPost=nPost)
        xa, xb = xb, xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N) if x0 is None else x0), bd, xb, ncyc, nPre=nPre, nPost=nPost)
    xl = xb.download()
    out = (x, xl, H.dictionary_levels(), H.paired_levels(nPre), H.paired_levels(nPost, "up"))
    H.free()
    return out


def _on_off(mg, U, sweeps=(3, 3), **kw):
    x1, xl1, lv1, pd1, pu1 = _run(mg, U, True, sweeps, **kw)
    x0, xl0, lv0, _, _ = _run(mg, U, False, sweeps, **kw)
    assert lv0 == {}, lv0
    assert _same(x1, x0), float(np.max(np.abs(x1 - x0)))
    assert _same(xl1, xl0) and _same(xl1, x1)
    return lv1, pd1, pu1


CASES = [
    (64, (4, 2, 2), (3, 3), None),            # levels smaller than one tile
    (256, (4, 2, 2), (3, 3), None),
    (256, (4, 2, 2), (3, 3), DIR_NEU),
    (4096, (4, 2, 2), (3, 3), None),
    (4096, (4, 2, 2), (3, 3), DIR_NEU),
    (4096 + 512, (4, 2, 2), (1, 2), None),    # tiles cut by the domain end
    (3072, (4, 2, 2), (3, 3), None),          # 61 / 55 classes, non-dyadic
    (2**14, (4, 4, 4), (3, 3), None),
    (2**13, (2, 2, 2, 2), (2, 1), None),      # levels 1 + 2 paired, level 3 alone
    (3 * 2**10, (4, 2, 4), (4, 4), None),
]


@pytest.mark.parametrize("n,ratios,sweeps,bc", CASES,
                         ids=[f"n{n}-r{''.join(map(str, r))}-V{s[0]}{s[1]}-{'dirneu' if bc else 'default'}" for n, r, s, bc in CASES])
def test_cycles_bitwise(mg, n, ratios, sweeps, bc):
    """1. on / off bitwise, pairing on; the paired launch is the one under test and both of its levels have a dictionary"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=ratios, bc=bc)
    cpu = {k: _cpu_classes(U, k) for k in (1, 2)}
    ne = {k: U.levels[k]["ne"] for k in (1, 2)}
    lv, pd, pu = _on_off(mg, U, sweeps)
    print(f"n={n} ratios={ratios} V{sweeps}: device classes per level {lv}, CPU input classes {cpu}, elements {ne}, "
          f"paired down {pd} up {pu}")
    # (the ascent pairs from the coarse side: levels 2 + 3 of the five-level hierarchy, level 1 alone)
    assert pd == [1] and pu == ([2] if len(ratios) == 4 else [1]), (pd, pu)
    for k in (1, 2):
        assert k in lv and 1 <= lv[k] <= min(ne[k], 1024), (lv, ne)
        assert lv[k] >= cpu[k], (lv, cpu)


def test_halves_and_nonzero_guess_bitwise(mg):
    """2. the descent alone from a random guess (the coarsest right-hand side compared), the ascent alone after a cycle"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(4096, p=3, pAgg=1, ratios=RATIOS)
    b = U.rhs()
    g = np.random.default_rng(7).standard_normal(len(b))
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        assert (1 in H.dictionary_levels() and 2 in H.dictionary_levels()) == on
        bd, xd = ctx.to_device(b), ctx.alloc(len(b))
        H.vcycle_down_dev(ctx.to_device(g), bd)
        rhs_ptr, _, nc = H.coarse_buffers()
        rc = np.empty(nc)
        ctx.synchronize()
        ctx.check(ctx.lib.aggmg_memcpy_d2h(ctx.handle, rc.ctypes.data, rhs_ptr, nc * 8))
        res = [rc]
        H.vcycle_dev(ctx.to_device(g), bd, xd)   # (leaves a coarsest solution for the ascent alone)
        res.append(xd.download())
        H.vcycle_up_dev(bd, xd)
        res.append(xd.download())
        out.append(res)
        H.free()
    for r1, r0 in zip(*out):
        assert _same(r1, r0)
    assert np.any(out[0][0] != 0.0)


@pytest.mark.parametrize("n", [4096, 3072])
def test_pairing_and_dictionary_combinations_bitwise(mg, n):
    """3. AGGMG_OPT_PAIR_LEVELS x AGGMG_OPT_OPERATOR_DICTIONARY: four runs, one result"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=RATIOS)
    runs = {(pair, on): _run(mg, U, on, pair=pair) for pair in (True, False) for on in (True, False)}
    base = runs[(True, True)]
    assert base[3] == [1] and base[4] == [1] and 1 in base[2] and 2 in base[2], base[2:]
    for key, r in runs.items():
        assert (r[3] == [1]) == key[0] and (r[2] != {}) == key[1], (key, r[2:])
        assert _same(r[0], base[0]) and _same(r[1], base[1]), key


def test_level_without_the_form_bitwise(mg):
    """4. a uniform mesh of an interval whose vertices round in many different ways (the mesh that overflows the fine
    level's dictionary): whatever the class counts of levels 1 and 2 are, on / off are bitwise equal; a level with more
    than 1024 CPU classes has no dictionary, and a pair with one dictionary only runs the full arrays"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(160000, p=3, pAgg=1, ratios=RATIOS, xin=-1.0 / 3.0, xout=1.0e9 + 0.7)
    cpu = {k: _cpu_classes(U, k) for k in (1, 2)}
    lv, pd, pu = _on_off(mg, U, ncyc=2)
    print(f"CPU input classes {cpu}, device classes {lv}")
    assert pd == [1] and pu == [1]
    for k in (1, 2):
        if cpu[k] > 1024:
            assert k not in lv, (cpu, lv)
        if k in lv:
            assert cpu[k] <= lv[k] <= 1024, (cpu, lv)


def test_sweep_weights_bitwise(mg):
    """5. a weight schedule on each of the two levels of the paired launch"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(4096, p=3, pAgg=1, ratios=RATIOS)
    weights = {1: ([0.5, 0.9, 1.3], [1.1, 0.7, 0.6]), 2: ([0.8, 1.2, 0.55], [0.95, 0.65, 1.05])}
    lv, pd, pu = _on_off(mg, U, weights=weights)
    assert pd == [1] and pu == [1] and 1 in lv and 2 in lv, (lv, pd, pu)
    x_w = _run(mg, U, True, weights=weights)[0]
    x_p = _run(mg, U, True)[0]
    assert not _same(x_w, x_p), "the schedule changed nothing: it did not reach the launch under test"
