"""Element-thread form of the two-level dictionary launches (csrc/pair_elem_kernels.hpp, btd_pair_down_elem_kernel /
btd_pair_up_elem_kernel; AGGMG_OPT_PAIR_ELEMENT_THREADS): one thread owns an element of each of the launch's two levels,
the class records of both levels lie in LDS.  The kernels repeat the row-thread dictionary kernels' expressions, so every
result must equal BIT FOR BIT the row-thread dictionary kernels' (new option off) and the plain kernels' (dictionary off),
compared as 64-bit patterns.  Three arms per case, each running vcycle_dev x 3 and vcycles_dev(3).

The launch counter (aggmg_pair_element_thread_launches) is asserted exactly: one per two-level launch both of whose
levels have at most CAP classes, none with the option or the dictionary off; the fine level's counter
(aggmg_element_thread_launches) does not depend on the new option."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)
TEA, TEB = 256, 128                         # kPairElemTEA, kPairElemTEB: what the planners are given
CAP = 32                                    # kPairElemMaxClasses
NCYC = 3


def pair_down_plan(npre, rho_ab, rho_bc, tea=TEA, teb=TEB):
    """host_plan.hpp pair_down_plan -> (own [level-b elements], te_a, te_b)"""
    hh = npre + 1
    te_b = min(teb, (tea - 2 * hh) // rho_ab)
    own = ((te_b - 2 * hh) // rho_bc) * rho_bc
    return (own, (own + 2 * hh) * rho_ab + 2 * hh, own + 2 * hh) if own > 0 else (0, 0, 0)


def pair_up_plan(npost, rho_ab, tea=TEA, teb=TEB):
    """host_plan.hpp pair_up_plan -> (own [level-a elements], te_a, te_b)"""
    hb = (npost + rho_ab - 1) // rho_ab
    own = (min(tea - 2 * npost, (teb - 2 * hb - 2 * npost) * rho_ab) // rho_ab) * rho_ab
    return (own, own + 2 * npost, own // rho_ab + 2 * hb + 2 * npost) if own > 0 else (0, 0, 0)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def arms(mg):
    """the three contexts: element threads / row threads (both with the dictionary) / the plain kernels"""
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    for name, d, e in (("elem", 1, 1), ("row", 1, 0), ("plain", 0, 1)):
        ctx = mg.Context(0)
        ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, d)
        ctx.set_option(_lib.OPT_PAIR_LEVELS, 1)
        ctx.set_option(_lib.OPT_PAIR_ELEMENT_THREADS, e)
        out[name] = ctx
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(ctx, U, sweeps, x0, weights):
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    npre, npost = sweeps
    H = build_device_hierarchy(U, ctx)
    if weights:
        for k, (pre, post) in weights.items():
            H.set_sweep_weights(k, pre, post)
    b = U.rhs()
    N = len(b)
    bd = ctx.to_device(b)
    k0, f0 = ctx.pair_element_thread_launches(), ctx.element_thread_launches()
    xa, xb = ctx.to_device(np.zeros(N) if x0 is None else x0), ctx.alloc(N)
    for _ in range(NCYC):
        H.vcycle_dev(xa, bd, xb, nPre=npre, nPost=npost)
        xa, xb = xb, xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N) if x0 is None else x0), bd, xb, NCYC, nPre=npre, nPost=npost)
    xl = xb.download()
    out = dict(x=x, xl=xl, lv=H.dictionary_levels(), pd=H.paired_levels(npre), pu=H.paired_levels(npost, "up"),
               pair=ctx.pair_element_thread_launches() - k0, fine=ctx.element_thread_launches() - f0)
    H.free()
    return out


def _expected(lv, pd, pu):
    """two-level launches of one cycle whose two levels both have a dictionary of at most CAP classes"""
    return sum(1 for k in list(pd) + list(pu) if 0 < lv.get(k, 0) <= CAP and 0 < lv.get(k + 1, 0) <= CAP)


def _three(arms, U, sweeps=(3, 3), x0=None, weights=None, under_cap=None):
    e = _run(arms["elem"], U, sweeps, x0, weights)
    r = _run(arms["row"], U, sweeps, x0, weights)
    p = _run(arms["plain"], U, sweeps, x0, weights)
    per_cycle = _expected(e["lv"], e["pd"], e["pu"])
    print(f"classes {e['lv']} paired down {e['pd']} up {e['pu']}: element-thread pair launches {e['pair']} "
          f"(expected {2 * NCYC} x {per_cycle}), fine-level element-thread launches {e['fine']}")
    assert p["lv"] == {} and e["lv"] == r["lv"], (e["lv"], r["lv"], p["lv"])
    assert e["pd"] and e["pu"] and e["pd"] == r["pd"] == p["pd"] and e["pu"] == r["pu"] == p["pu"]
    if under_cap is not None:
        assert (per_cycle == len(e["pd"]) + len(e["pu"])) == under_cap, (e["lv"], per_cycle)
    assert e["pair"] == 2 * NCYC * per_cycle, (e["pair"], per_cycle)
    assert r["pair"] == 0 and p["pair"] == 0, (r["pair"], p["pair"])
    assert e["fine"] == r["fine"] and p["fine"] == 0 and (e["fine"] > 0) == (0 in e["lv"]), (e["fine"], r["fine"], p["fine"])
    assert np.all(np.isfinite(p["x"])) and np.any(p["x"] != 0.0)
    for what, got, ref in (("elem / plain", e["x"], p["x"]), ("row / plain", r["x"], p["x"]),
                           ("elem / plain, loop", e["xl"], p["xl"]), ("row / plain, loop", r["xl"], p["xl"])):
        assert _same(got, ref), (what, float(np.max(np.abs(got - ref))))
    assert _same(e["xl"], e["x"])
    return e


def _hier(n, ratios=RATIOS, bc=None, few_classes=False):
    """few_classes: the interval [2^20, 2^20 + n] -- a mesh width of 1 and vertices that all round alike, so the records
    repeat (5 distinct input records per level) and the levels stay under the class cap at an n that is no power of two"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    kw = dict(xin=2.0**20, xout=2.0**20 + n) if few_classes else {}
    return UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=ratios, bc=bc, **kw)


CASES = [
    (64, (4, 2, 2), (3, 3), None),            # levels smaller than one tile
    (256, (4, 2, 2), (3, 3), None),
    (256, (4, 2, 2), (3, 3), DIR_NEU),
    (4096, (4, 2, 2), (3, 3), None),
    (3072, (4, 2, 2), (3, 3), None),
    (2**14, (4, 4, 4), (3, 3), None),
    (2**13, (2, 2, 2, 2), (2, 1), None),      # descent: levels 1 + 2, ascent: levels 2 + 3
    (3 * 2**10, (4, 2, 4), (4, 4), None),
]


@pytest.mark.parametrize("n,ratios,sweeps,bc", CASES,
                         ids=[f"n{n}-r{''.join(map(str, r))}-V{s[0]}{s[1]}-{'dirneu' if bc else 'default'}" for n, r, s, bc in CASES])
def test_cycles_bitwise(mg, arms, n, ratios, sweeps, bc):
    """the shapes of tests/test_gpu_pair_dictionary.py; the counter follows the class counts of the case"""
    _three(arms, _hier(n, ratios, bc), sweeps)


def _edge_sizes():
    """fine sizes n (ratios 4, 2, 2, V(3,3)) whose level-b / level-a tile count is k and k + 1 at the 1 -> 2 and 2 -> 3
    steps of the descent's plan (own level-b elements, n = 8 ne_b) and of the ascent's (own level-a elements, n = 4 ne_a)"""
    own_d, own_u = pair_down_plan(3, 2, 2)[0], pair_up_plan(3, 2)[0]
    ns = set()
    for k in (1, 2):
        for own, per in ((own_d, 8), (own_u, 4)):
            last = -(-(k * own * per) // 16) * 16          # n a multiple of 16: the first size past k tiles ...
            if last == k * own * per:
                last += 16
            ns.update((last - 16, last))                    # ... and the last size of k tiles
    return own_d, own_u, sorted(ns)


OWN_D, OWN_U, EDGE_NS = _edge_sizes()


def test_planner_tiles():
    """what the edge sizes are derived from"""
    print(f"descent own {OWN_D} level-b elements, ascent own {OWN_U} level-a elements; n: {EDGE_NS}")
    assert pair_down_plan(3, 2, 2) == (116, 256, 124) and pair_up_plan(3, 2) == (236, 242, 128)
    for k in (1, 2):
        assert any(-(-(n // 8) // OWN_D) == k for n in EDGE_NS) and any(-(-(n // 8) // OWN_D) == k + 1 for n in EDGE_NS)
        assert any(-(-(n // 4) // OWN_U) == k for n in EDGE_NS) and any(-(-(n // 4) // OWN_U) == k + 1 for n in EDGE_NS)


@pytest.mark.parametrize("n", EDGE_NS)
def test_tile_count_edges_bitwise(mg, arms, n):
    """one, two and three tiles per level, the last one owning a few elements or a whole range; the element-thread
    kernels must run (both levels under the cap)"""
    _three(arms, _hier(n, few_classes=True), under_cap=True)


@pytest.mark.parametrize("sweeps", [(1, 1), (8, 8)])
def test_sweep_counts_bitwise(mg, arms, sweeps):
    """the smallest and the largest halo the two-level launches take"""
    e = _three(arms, _hier(4096), sweeps, under_cap=True)
    assert e["pd"] == [1] and e["pu"] == [1]


def test_initial_guess_bitwise(mg, arms):
    U = _hier(4096)
    g = np.random.default_rng(7).standard_normal(len(U.rhs()))
    _three(arms, U, x0=g, under_cap=True)


def test_sweep_weights_bitwise(mg, arms):
    """a weight schedule on each of the two levels of the paired launch"""
    weights = {1: ([0.5, 0.9, 1.3], [1.1, 0.7, 0.6]), 2: ([0.8, 1.2, 0.55], [0.95, 0.65, 1.05])}
    U = _hier(4096)
    e = _three(arms, U, weights=weights, under_cap=True)
    assert not _same(e["x"], _run(arms["elem"], U, (3, 3), None, None)["x"]), "the schedule did not reach the launch"


def test_over_the_cap_keeps_row_threads(mg, arms):
    """133 / 117 classes on the two levels: over the cap, no element-thread pair launch, the same bits"""
    e = _three(arms, _hier(4096 + 512), (1, 2), under_cap=False)
    assert e["lv"][1] > CAP and e["lv"][2] > CAP and e["pair"] == 0, e["lv"]
