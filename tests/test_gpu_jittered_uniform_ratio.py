"""The uniform-ratio fused kernels -- btd_fused_kernel with one agglomeration ratio, the two-level btd_pair_down /
btd_pair_up, their dictionary and element-thread forms, the K-column block-tridiagonal kernel, the checkpoint variant of
multigrid and the replayed ascent -- on meshes whose elements are all unequal (tests/jitter_helpers.py): every interior
vertex moved by a seeded +-0.3 of the element width, one agglomerate size per level.  The device takes the ratio from the
transfer's structure, so these hierarchies reach the rho > 0 instantiations with every element's operator record,
inverse block and transfer block distinct: a thread that loads a neighbour's record, which no uniform mesh can show
(tests/test_jitter_sensitivity_cpu.py: the change is exactly 0 or 1e-16 there), moves the result by 3e-8 .. 1e-2 of the
scale here, against a bound of 1e-12.

Operators come from the oracle's builders through MeshHierarchy.from_reference and from build_device_ragged_hierarchy
with a single agglomerate size; nothing is called below the public entry points.  Every arm is a context of its own
with its options set before the hierarchy is made, and every arm asserts which kernel family ran (_expected,
_launch_counts).

What the set-up declines on these operators, asserted as it is:
 * the element-thread form of the two-level launches takes levels of at most 32 distinct records (kPairElemMaxClasses);
   a jittered level of 96 .. 1024 elements has as many records as elements, so its counter stays 0 in every arm and the
   two-level launches run their row-thread dictionary and plain forms;
 * the element-thread kernel of the fine level, and with it the replayed ascent, needs a dictionary on a fine level of
   4-row blocks: c34_small only (c34's fine level has 2048 > 1024 records; b2, p2, b8 have other block sizes);
 * with one coarse row per agglomerate (b2, pAgg = 0) the agglomerated levels have blocks of one row: no dictionary, no
   two-level launch and no K-column launch takes them, on any mesh; b2 runs btd_fused_kernel level by level, its
   K-column cycle column by column;
 * with the symmetric packing off there are neither dictionaries nor two-level launches (both read the packed inverses).
The symmetric form of the residual is not declined: the fine level of p = 3 takes it, as on a uniform mesh.

Bounds (jitter_helpers): ||A (x - x_ref)|| <= 1e-12 (||b|| + ||A x0||) everywhere (reference against reference, sparse
against dense LU at the coarsest level, on these inputs: at most 4.7e-15; measured on the device: at most 2.3e-14);
||x - x_ref|| <= 1e-10 ||x_ref|| for one cycle and for the first cycle of a loop; from the second cycle of a loop on the
reference differs from itself by up to 3.6e-10 in the iterate (4.7e-15 in the residual), so that bound is not the
reference's to give there and ten times its own figure stands in (loop_iterate_tol; measured on the device: at most
6.4e-10); residual histories rtol 1e-8, atol 1e-11 max(||b||, res[0]) (reference against reference: 6e-13 relative)."""
import numpy as np
import pytest

import jitter_helpers as jh
from test_gpu_multi_rhs import _multi, _single

pytestmark = pytest.mark.gpu

ARMS = ("default", "no_dict", "no_dict_no_pair", "row_threads", "store", "no_sym")
SWEEPS = {"c34": ((3, 3), (1, 2), (0, 3), (8, 8))}
SEED = jh.X0_SEED


def _arm_options(arm):
    from agglomerationmultigrid1d_amd import _lib
    return {
        "default": {},
        "no_dict": {_lib.OPT_OPERATOR_DICTIONARY: 0},
        "no_dict_no_pair": {_lib.OPT_OPERATOR_DICTIONARY: 0, _lib.OPT_PAIR_LEVELS: 0},
        "row_threads": {_lib.OPT_ELEMENT_THREADS: 0, _lib.OPT_PAIR_ELEMENT_THREADS: 0},
        "store": {_lib.OPT_REPLAY_PRESMOOTH: 0},
        "no_sym": {_lib.OPT_SYMMETRIC_PACKING: 0, _lib.OPT_SYMMETRIC_RESIDUAL: 0},
    }[arm]


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


class _World:
    """reference hierarchies and cycles (once per case), contexts (once per arm), device hierarchies (once per case and
    arm); the reference's arrays stay as built (the control test undoes its change before it returns)"""

    def __init__(self, oracle, mg):
        self.o, self.mg = oracle, mg
        self.refs, self.ctxs, self.hiers = {}, {}, {}

    def ref(self, case):
        if case not in self.refs:
            o = self.o
            Ho, b = jh.build(o, case, True)
            N = len(b)
            A = Ho.mStiffness[0]
            x0 = o.splitmix_normal(N, SEED)
            r = dict(Ho=Ho, b=b, A=A, N=N, x0=x0, one={}, ne=[S.mBlockInds.shape[1] for S in Ho.mSmoothers])
            for nPre, nPost in SWEEPS.get(case, ((3, 3),)):
                r["one"][nPre, nPost] = o.multigrid_v_cycle(Ho, x0, b, nPre=nPre, nPost=nPost, alpha=jh.ALPHA)
            xs, res, x = [], [], np.zeros(N)
            for _ in range(jh.NCYC):
                x = o.multigrid_v_cycle(Ho, x, b)
                xs.append(x)
                res.append(float(np.linalg.norm(A @ x - b)))
            r["xs"], r["res"] = xs, res
            if case in jh.MULTI_CASES:
                B, X0 = jh.columns(o, b, 8, jh.MULTI_SEED)
                r["B"], r["X0"] = B, X0
                r["XR"] = np.column_stack([o.multigrid_v_cycle(Ho, X0[:, j], B[:, j]) for j in range(8)])
            self.refs[case] = r
        return self.refs[case]

    def ctx(self, arm):
        if arm not in self.ctxs:
            c = self.mg.Context(0)
            for opt, v in _arm_options(arm).items():
                c.set_option(opt, v)
            self.ctxs[arm] = c
        return self.ctxs[arm]

    def hier(self, case, arm):
        if (case, arm) not in self.hiers:
            self.hiers[case, arm] = self.mg.MeshHierarchy.from_reference(self.ref(case)["Ho"], ctx=self.ctx(arm))
        return self.hiers[case, arm]

    def close(self):
        for H in self.hiers.values():
            H.free()


@pytest.fixture(scope="module")
def world(oracle, mg):
    w = _World(oracle, mg)
    yield w
    w.close()


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


FIGURES = {}     # (what, case, arm) -> largest ||A (x - x_ref)|| / scale seen, printed by the last test


def _assert_rule_1(r, x, xr, b, x0, iterate_tol, what):
    """||A (x - x_ref)|| <= 1e-12 (||b|| + ||A x0||) and ||x - x_ref|| <= iterate_tol ||x_ref||, figures printed first"""
    A = r["A"]
    scale = float(np.linalg.norm(b) + (np.linalg.norm(A @ x0) if x0 is not None else 0.0))
    res = float(np.linalg.norm(A @ (x - xr))) / scale
    rel = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    print(f"[jittered] {what}: ||A (x - x_ref)|| / scale = {res:.3e}   ||x - x_ref|| / ||x_ref|| = {rel:.3e}")
    FIGURES[what[:3]] = max(FIGURES.get(what[:3], 0.0), res)
    assert np.all(np.isfinite(x)), what
    assert res <= jh.RESIDUAL_TOL, (what, res)
    assert rel <= iterate_tol, (what, rel, iterate_tol)


# ---- which family ran ----------------------------------------------------------------------------------------------------
def _facts(H, ne):
    """what the set-up chose for a hierarchy, as its reports give it"""
    lv = H.dictionary_levels()
    return dict(kinds=H.level_kinds(), dictionary=sorted(lv), every_record_distinct=all(lv[k] == ne[k] for k in lv),
                paired_down=H.paired_levels(3, "down"), paired_up=H.paired_levels(3, "up"), sym_residual=H.sym_residual_levels())


def _expected(case, arm, nlev):
    """What the set-up chooses, by its own rules (the same choices as on a uniform mesh of the shape, but for the record
    counts): every smoothed level on the fused block-tridiagonal kernels.
     * Dictionary: a level of at most 1024 distinct records, here as many as it has elements -- the agglomerated levels
       with two coarse rows per agglomerate (pAgg = 1), and the fine level where its blocks have 4 rows (c34_small); it
       indexes the packed symmetric inverse blocks, so none with the packing off.
     * Two levels per launch: levels 1 and 2 of a hierarchy with a level 2 above the coarsest, blocks of 2 rows, packed
       symmetric inverses, two-mode transfers of one ratio -- c34, c34_small, p2; not b8 (three levels), not b2 (one coarse
       row per agglomerate: blocks of one row), not with the packing off.
     * Symmetric form of the residual: the fine level of p = 3 (tests/test_gpu_sym_residual.py: blocks of 4 rows only).
       The jittered entries do mirror closely enough for it: it is not declined."""
    n, p, pAgg, _, first = jh.CASES[case]
    ne = [n] + [n // first // 2 ** i for i in range(nlev - 2)]
    packed = arm != "no_sym"
    dictionary = []
    if packed and arm not in ("no_dict", "no_dict_no_pair") and pAgg == 1:
        dictionary = [k for k in range(nlev - 1) if ne[k] <= 1024 and (k >= 1 or p == 3)]
    pair = packed and arm != "no_dict_no_pair" and pAgg == 1 and nlev >= 4
    return dict(kinds=["fused_btd"] * (nlev - 1) + ["coarsest"], dictionary=dictionary, every_record_distinct=True,
                paired_down=[1] if pair else [], paired_up=[1] if pair else [],
                sym_residual=[0] if p == 3 and packed else [])


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case", list(jh.CASES))
def test_families(world, case, arm):
    """the set-up's choices on the jittered operators, arm by arm: the families of the module docstring ran"""
    r = world.ref(case)
    H = world.hier(case, arm)
    facts = _facts(H, r["ne"])
    print(f"[jittered] families {case} {arm}: {facts} records {H.dictionary_levels()} elements {r['ne']}")
    assert facts == _expected(case, arm, len(r["ne"])), (case, arm)
    if case == "c34" and arm == "default":
        assert facts["dictionary"] == [1, 2] and facts["paired_down"] == [1]
    if case == "c34_small" and arm == "default":
        assert facts["dictionary"] == [0, 1, 2]
    if arm in ("no_dict", "no_dict_no_pair"):
        assert H.dictionary_levels() == {}


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case", list(jh.CASES))
def test_launches_follow_the_reports(world, case, arm):
    """one profiled V(3,3): every smoothed level runs one fused launch each way, but the second level of a reported
    pair, which runs none (as tests/test_gpu_ratio_regimes.py::test_pairing_reports_are_truthful)"""
    r = world.ref(case)
    H = world.hier(case, arm)
    ctx = H.ctx
    db, dx0, dx = ctx.to_device(r["b"]), ctx.to_device(r["x0"]), ctx.alloc(r["N"])
    H.vcycle_dev(dx0, db, dx, 3, 3, jh.ALPHA)      # work space allocated outside the profiled call
    ctx.synchronize()
    ctx.profile_enable(True)
    try:
        H.vcycle_dev(dx0, db, dx, 3, 3, jh.ALPHA)
        stats = ctx.profile_collect()
    finally:
        ctx.profile_enable(False)
    print(f"[jittered] launches {case} {arm}: {sorted((k, v[1]) for k, v in stats.items())}")
    for kind, direction in (("fused_down", "down"), ("fused_up", "up")):
        paired = H.paired_levels(3, direction)
        for k in range(H.nlevels - 1):
            assert stats.get((kind, k), (0.0, 0))[1] == (0 if (k - 1) in paired else 1), (kind, k, paired, stats)
    assert ("residual", 0) not in stats and ("prolong", 0) not in stats, stats


def _launch_counts(case, arm):
    """(element-thread launches, two-level element-thread launches, replayed cycles) of one V(3,3) through vcycle_dev.
    The element-thread kernel runs a fine level of 4-row blocks that has a dictionary, once down and once up: c34_small
    with the dictionary, the packing and the option on; its ascent replays the pre-smoothing unless told to store.  c34's
    fine level has 2048 > 1024 records and no dictionary, so neither runs there at any sweep count.  The element-thread
    form of the two-level launches takes levels of at most 32 records: never on a jittered level of 96 and more."""
    elem = case == "c34_small" and arm in ("default", "store")
    return (2 if elem else 0), 0, (1 if elem and arm == "default" else 0)


# ---- 1. one cycle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case,sweeps", [(c, s) for c in jh.CASES for s in SWEEPS.get(c, ((3, 3),))],
                         ids=[f"{c}-V{s[0]}{s[1]}" for c in jh.CASES for s in SWEEPS.get(c, ((3, 3),))])
def test_one_cycle_against_the_oracle(mg, world, case, sweeps, arm):
    r = world.ref(case)
    H = world.hier(case, arm)
    ctx = H.ctx
    nPre, nPost = sweeps
    b, x0, N = r["b"], r["x0"], r["N"]
    before = (ctx.element_thread_launches(), ctx.pair_element_thread_launches(), ctx.replay_launches())
    dx = ctx.alloc(N)
    H.vcycle_dev(ctx.to_device(x0), ctx.to_device(b), dx, nPre, nPost, jh.ALPHA)
    x = dx.download()
    grown = tuple(a - b_ for a, b_ in zip((ctx.element_thread_launches(), ctx.pair_element_thread_launches(), ctx.replay_launches()), before))
    print(f"[jittered] {case} {arm} V({nPre},{nPost}): element-thread / two-level element-thread / replay launches {grown}")
    _assert_rule_1(r, x, r["one"][sweeps], b, x0, jh.ITERATE_TOL, ("one cycle", case, arm, sweeps))
    # the host-pointer form: the same bits
    xh = mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost, alpha=jh.ALPHA)
    assert _same(xh, x), float(np.max(np.abs(xh - x)))
    assert grown == _launch_counts(case, arm), (case, arm, sweeps, grown)


@pytest.mark.parametrize("arm", ("default", "no_dict"))
@pytest.mark.parametrize("level", (0, 1, 2))
def test_the_comparison_sees_a_neighbours_transfer_block(mg, oracle, world, level, arm):
    """the control: a hierarchy whose transfer carries the neighbour agglomerate's block at one agglomerate of one level
    (jitter_helpers.neighbour_transfer_block) goes to the device.  Its cycle is the oracle's cycle of that hierarchy to
    the bound -- and misses the unchanged oracle's by 100 times the bound and more (5.0e-7 .. 1.7e-4 of the scale): what a
    kernel reading the wrong agglomerate's rows would compute does not pass test_one_cycle_against_the_oracle"""
    r = world.ref("c34")
    Ho, b, x0, N = r["Ho"], r["b"], r["x0"], r["N"]
    ctx = world.ctx(arm)
    with jh.neighbour_transfer_block(Ho, level):
        xm = oracle.multigrid_v_cycle(Ho, x0, b)
        H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
    try:
        assert H.level_kinds() == ["fused_btd"] * 3 + ["coarsest"] and H.paired_levels() == [1]
        dx = ctx.alloc(N)
        H.vcycle_dev(ctx.to_device(x0), ctx.to_device(b), dx, 3, 3, jh.ALPHA)
        x = dx.download()
    finally:
        H.free()
    scale = jh.cycle_scale(Ho, b, x0)
    own = float(np.linalg.norm(r["A"] @ (x - xm))) / scale
    other = float(np.linalg.norm(r["A"] @ (x - r["one"][3, 3]))) / scale
    print(f"[jittered] control, level {level} {arm}: against the oracle of the changed hierarchy {own:.3e}, of the unchanged one {other:.3e}")
    assert own <= jh.RESIDUAL_TOL and other >= 100.0 * jh.RESIDUAL_TOL, (own, other)


# ---- 2. loops -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case", list(jh.CASES))
def test_cycles_back_to_back(world, case, arm):
    """vcycles_dev(k), k = 1, 2, 3: every iterate against the oracle's cycle repeated; three cycles in one call are three
    separate calls bit for bit"""
    r = world.ref(case)
    H = world.hier(case, arm)
    ctx = H.ctx
    b, N = r["b"], r["N"]
    bd, z = ctx.to_device(b), ctx.to_device(np.zeros(N))
    dx = ctx.alloc(N)
    for k in (1, 2, 3):
        H.vcycles_dev(z, bd, dx, k, 3, 3, jh.ALPHA)
        x = dx.download()
        _assert_rule_1(r, x, r["xs"][k - 1], b, None, jh.loop_iterate_tol(k), ("loop", case, arm, k))
        rk = float(np.linalg.norm(r["A"] @ x - b))
        assert np.isclose(rk, r["res"][k - 1], rtol=1e-8, atol=1e-11 * max(np.linalg.norm(b), r["res"][0])), (k, rk, r["res"][k - 1])
    xa, xb = ctx.to_device(np.zeros(N)), ctx.alloc(N)
    for _ in range(3):
        H.vcycle_dev(xa, bd, xb, 3, 3, jh.ALPHA)
        xa, xb = xb, xa
    assert _same(xa.download(), x), float(np.max(np.abs(xa.download() - x)))


@pytest.mark.parametrize("arm", ("default", "no_dict"))
@pytest.mark.parametrize("case", list(jh.CASES))
def test_device_loop_with_checks(mg, world, case, arm):
    """multigrid_dev, the residual test formed inside the fine-level launch: a check after every cycle and after every
    third; the histories against ||A x_k - b|| of the reference, the last iterate against its fourth"""
    r = world.ref(case)
    H = world.hier(case, arm)
    ctx = H.ctx
    b, N, ref = r["b"], r["N"], np.asarray(r["res"])
    bd, z = ctx.to_device(b), ctx.to_device(np.zeros(N))
    atol = 1e-11 * max(np.linalg.norm(b), ref[0])
    out = {}
    for every, at in ((1, [0, 1, 2, 3]), (3, [2, 3])):
        dx, ncyc, res = mg.multigrid_dev(H, z, bd, jh.NCYC, 1e-30, check_every=every, nPre=3, nPost=3, alpha=jh.ALPHA)
        print(f"[jittered] {case} {arm} multigrid_dev check_every={every}: {ncyc} cycles, res {res} reference {ref[at].tolist()}")
        assert ncyc == jh.NCYC and len(res) == len(at)
        assert np.allclose(res, ref[at], rtol=1e-8, atol=atol)
        out[every] = dx.download()
        _assert_rule_1(r, out[every], r["xs"][-1], b, None, jh.loop_iterate_tol(jh.NCYC), ("device loop", case, arm, every))
    assert _same(out[1], out[3])


# ---- 3. K columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 8))
@pytest.mark.parametrize("arm", ("default", "no_dict"))
@pytest.mark.parametrize("case", jh.MULTI_CASES)
def test_k_columns(mg, world, case, arm, K):
    """vcycle_multi_dev on distinct columns: column groups reported, every column against the oracle's cycle of that
    column, every column the single-column call bit for bit.  b2 has one coarse row per agglomerate and the K-column
    kernel takes two-mode transfers only: its cycle is reported, and runs, column by column"""
    r = world.ref(case)
    H = world.hier(case, arm)
    ctx = H.ctx
    N = r["N"]
    B, X0 = r["B"][:, :K], r["X0"][:, :K]
    fused, group = H.multi_info(K, 3, 3)
    print(f"[jittered] {case} {arm} K={K}: multi_info {(fused, group)}")
    assert (fused, group) == ((True, K) if case == "c34" else (False, 1)), (fused, group)
    X = _multi(mg, H, ctx, X0, B, 3, 3, N + (K % 2))
    for j in range(K):
        _assert_rule_1(r, X[:, j], r["XR"][:, j], B[:, j], X0[:, j], jh.ITERATE_TOL, ("column", case, arm, K, j))
    R = _single(H, ctx, X0, B, 3, 3)
    for j in range(K):
        assert _same(X[:, j], R[:, j]), (j, float(np.max(np.abs(X[:, j] - R[:, j]))))


# ---- 4. level 2 over several tiles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("arm", ("default", "no_dict"))
@pytest.mark.parametrize("size", (4, 2))
def test_several_tiles_on_every_level(mg, world, size, arm):
    """2^14 jittered fine elements, agglomerates of one size (4: levels of 4096, 1024, 256 elements; 2: 8192, 4096, 2048)
    through the device set-up: the uniform-ratio path (a two-level launch needs one ratio) against the generic
    composition of the same operators, at the two bounds of test_ragged_agglomerates_at_size_fused_equals_unfused"""
    from agglomerationmultigrid1d_amd.uniform import build_device_ragged_hierarchy
    ctx = world.ctx(arm)
    H, b, info = build_device_ragged_hierarchy(2 ** 14, ctx, sizes=(size,), generic=True, seed=5)
    Hg = info["generic"]
    try:
        print(f"[jittered] ragged size {size} {arm}: {info['elements']} mean {info['mean_agglomerate']} kinds {H.level_kinds()} "
              f"paired {H.paired_levels()} dictionary {H.dictionary_levels()}")
        assert H.level_kinds() == ['fused_btd'] * 3 + ['coarsest'] and Hg.level_kinds() == ['generic'] * 3 + ['coarsest']
        assert H.paired_levels() == [1]
        assert info["mean_agglomerate"] == [float(size)] * 3 and info["elements"] == [2 ** 14 // size ** k for k in range(4)]
        if arm == "no_dict":
            assert H.dictionary_levels() == {}
        N = len(b)
        bd, z = ctx.to_device(b), ctx.to_device(np.zeros(N))
        xf, xg, rr = ctx.alloc(N), ctx.alloc(N), ctx.alloc(N)
        H.vcycle_dev(z, bd, xf)
        Hg.vcycle_dev(z, bd, xg)
        xfh, xgh = xf.download(), xg.download()
        d = ctx.to_device(xfh - xgh)
        ctx.check(ctx.lib.aggmg_residual_dev(ctx.handle, H._ops[0].handle, d.ptr, z.ptr, rr.ptr))
        res = float(np.linalg.norm(rr.download()) / np.linalg.norm(b))
        rel = float(np.linalg.norm(xfh - xgh) / np.linalg.norm(xfh))
        print(f"[jittered] ragged size {size} {arm}: ||A (xf - xg)|| / ||b|| = {res:.3e}   ||xf - xg|| / ||xf|| = {rel:.3e}")
        FIGURES["ragged", size, arm] = res
        assert np.all(np.isfinite(xfh)) and np.any(xfh != 0.0)
        assert res <= 1e-12 and rel <= 1e-10, (res, rel)
    finally:
        Hg.free()
        H.free()


def test_print_largest_figures():
    """the largest ||A (x - x_ref)|| / scale of every case and arm, for the record"""
    for key in sorted(FIGURES, key=str):
        print(f"[jittered] largest {key}: {FIGURES[key]:.3e}")
    assert all(v <= jh.RESIDUAL_TOL for v in FIGURES.values())
