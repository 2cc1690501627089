"""The kernels that read the operator through a table of class records in LDS -- the fine level's btd_elem_rec_kernel /
btd_elem_rec_replay_up_kernel (csrc/elem_kernels.hpp, AGGMG_OPT_ELEMENT_RECORDS_LDS) and the two-level
btd_pair_down_elem_kernel / btd_pair_up_elem_kernel (csrc/pair_elem_kernels.hpp), each taking levels of at most 32 classes
-- on PERIODIC, strongly non-uniform operators (tests/periodic_helpers.py), against the oracle.

tests/test_gpu_elem_records.py and tests/test_gpu_pair_elem.py run uniform meshes, where every interior element of a
level is in one class and a class index read at the wrong place gives the same bits, and compare option on with option
off, which agree when both share a wrong index.  tests/test_gpu_jittered_uniform_ratio.py gives every element a record of
its own: every level is over the cap and these kernels never run.  Here every level has few classes, every element's
class differs from both neighbours', and successive tiles start at different phases of the period
(tests/test_periodic_sensitivity_cpu.py: a neighbour's record at one element moves the cycle by 2e-7 of the scale and
more, against a bound of 1e-12).

Five arms, each a context of its own with its options set before the hierarchy is made:
    lds     defaults: records in LDS, element threads on the fine level and on the two-level launches, replayed ascent
    global  AGGMG_OPT_ELEMENT_RECORDS_LDS = 0: the fine level's element-thread kernels with the records from global memory
    row     AGGMG_OPT_ELEMENT_THREADS = 0, AGGMG_OPT_PAIR_ELEMENT_THREADS = 0: the row-thread dictionary kernels
    plain   AGGMG_OPT_OPERATOR_DICTIONARY = 0: no dictionary at all
    store   AGGMG_OPT_REPLAY_PRESMOOTH = 0: the storing descent and ascent
Every arm is held to the oracle first (_assert_rule_1); then the arms must agree as 64-bit patterns.  Every case asserts
its launch counters exactly (_launch_counts): no case falls back to the other kernels unseen.

Bounds (periodic_helpers, none of them from the device's results): ||A (x - x_ref)|| <= 1e-12 (||b|| + ||A x0||)
everywhere (reference against reference at most 4.3e-15); ||x - x_ref|| <= 4e-10 ||x_ref|| for one cycle, 2e-10 after the
first cycle of a loop -- ten times the reference's own 3.1e-11 and 1.3e-11, which are over a tenth of the project's 1e-10
on these meshes -- 4e-9 after later cycles (jitter_helpers.loop_iterate_tol; the reference: 1.2e-10) and 1e-10 for the
K-column test's columns (the reference: 2.4e-13); residual histories rtol 1e-8, atol 1e-11 max(||b||, res[0]).

Measured on the device: class counts per level 0 / 1 / 2, equal to the host-side proxy's at both sizes: period 3: 17 / 26 / 23,
period 5: 28 / 20 / 17.  Launches of one V(3,3), V(1,2) or V(2,3) (element-thread, of them records in LDS, two-level
element-thread, replayed): lds (2, 2, 2, 1), global (2, 0, 2, 1), row and plain (0, 0, 0, 0), store (2, 2, 2, 0); of V(8,8):
lds and store (1, 1, 2, 0), global (1, 0, 2, 0).  ||A (x - x_ref)|| / scale at most 3.7e-15 for one cycle, 2.2e-15 in the
loops, 2.1e-14 for the columns, in every arm alike (the arms agree as bits).  ||x - x_ref|| / ||x_ref||: one cycle
3.2e-11 of 4e-10, first cycle of a loop 7.3e-13 of 2e-10, later cycles 1.2e-10 of 4e-9, columns 6.1e-11 of 1e-10.  The
controls: 2.6e-16 .. 2.7e-14 against the oracle of the changed hierarchy, 9.1e-7 .. 2.7e-4 against the unchanged one."""
import contextlib

import numpy as np
import pytest

import jitter_helpers as jh
import periodic_helpers as ph
from test_gpu_multi_rhs import _multi, _single

pytestmark = pytest.mark.gpu

ARMS = ("lds", "global", "row", "plain", "store")
COUNTERS = ("element_thread_launches", "element_record_lds_launches", "pair_element_thread_launches", "replay_launches")


def _arm_options(arm):
    from agglomerationmultigrid1d_amd import _lib
    return {
        "lds": {},
        "global": {_lib.OPT_ELEMENT_RECORDS_LDS: 0},
        "row": {_lib.OPT_ELEMENT_THREADS: 0, _lib.OPT_PAIR_ELEMENT_THREADS: 0},
        "plain": {_lib.OPT_OPERATOR_DICTIONARY: 0},
        "store": {_lib.OPT_REPLAY_PRESMOOTH: 0},
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
            Ho, b = ph.build(o, case)
            N = len(b)
            A = Ho.mStiffness[0]
            x0 = o.splitmix_normal(N, ph.X0_SEED)
            r = dict(Ho=Ho, b=b, A=A, N=N, x0=x0, one={}, ne=[S.mBlockInds.shape[1] for S in Ho.mSmoothers])
            for sweeps in ph.sweeps_of(case):
                for start in ("x0", "none"):
                    r["one"][sweeps, start] = o.multigrid_v_cycle(Ho, x0 if start == "x0" else np.zeros(N), b, nPre=sweeps[0],
                                                                  nPost=sweeps[1], alpha=ph.ALPHA)
            xs, res, x = [], [], np.zeros(N)
            for _ in range(ph.NCYC):
                x = o.multigrid_v_cycle(Ho, x, b)
                xs.append(x)
                res.append(float(np.linalg.norm(A @ x - b)))
            r["xs"], r["res"] = xs, res
            if case == ph.MULTI_CASE:
                B, X0 = jh.columns(o, b, ph.MULTI_K, ph.MULTI_SEED)
                r["B"], r["X0"] = B, X0
                r["XR"] = np.column_stack([o.multigrid_v_cycle(Ho, X0[:, j], B[:, j]) for j in range(ph.MULTI_K)])
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


def _counters(ctx):
    return tuple(getattr(ctx, name)() for name in COUNTERS)


def _grown(ctx, before):
    return tuple(a - b for a, b in zip(_counters(ctx), before))


FIGURES = {}     # (what, case, arm) -> (largest ||A (x - x_ref)|| / scale, largest ||x - x_ref|| / ||x_ref||), printed at the end


def _assert_rule_1(r, x, xr, b, x0, iterate_tol, what):
    """||A (x - x_ref)|| <= 1e-12 (||b|| + ||A x0||) and ||x - x_ref|| <= iterate_tol ||x_ref||, figures printed first"""
    A = r["A"]
    scale = float(np.linalg.norm(b) + (np.linalg.norm(A @ x0) if x0 is not None else 0.0))
    res = float(np.linalg.norm(A @ (x - xr))) / scale
    rel = float(np.linalg.norm(x - xr) / np.linalg.norm(xr))
    print(f"[periodic] {what}: ||A (x - x_ref)|| / scale = {res:.3e}   ||x - x_ref|| / ||x_ref|| = {rel:.3e}  (bound {iterate_tol:.1e})")
    old = FIGURES.get(what[:3], (0.0, 0.0))
    FIGURES[what[:3]] = (max(old[0], res), max(old[1], rel / iterate_tol))
    assert np.all(np.isfinite(x)), what
    assert res <= ph.RESIDUAL_TOL, (what, res)
    assert rel <= iterate_tol, (what, rel, iterate_tol)


# ---- which kernels run ------------------------------------------------------------------------------------------------------
def _launch_counts(arm, sweeps):
    """(element-thread launches, of them with the records in LDS, two-level element-thread launches, replayed cycles) of
    one vcycle_dev.  The fine level has 4-row blocks, a dictionary and at most 32 classes: its descent and its ascent
    are one element-thread launch each unless the option or the dictionary is off, with the records in LDS unless that
    option is 0.  Levels 1 and 2 go in one two-level launch each way, both under 32 classes: the element-thread form
    unless its option or the dictionary is off.  The ascent replays the pre-smoothing where the element-thread kernel
    runs, the option is on and the cycle's sweeps have a weight each (nPre + nPost <= 8).  V(8,8) is over that: it keeps
    the storing launches, and of its two fine-level launches the counters show one on the element-thread kernel (8
    sweeps and the residual behind them are more than one such launch fuses: that half keeps the row-thread kernel)."""
    elem = arm in ("lds", "global", "store")
    replay = elem and arm != "store" and sum(sweeps) <= 8
    fine = (1 if sweeps == (8, 8) else 2) if elem else 0
    return fine, (fine if arm in ("lds", "store") else 0), (2 if elem else 0), (1 if replay else 0)


@pytest.mark.parametrize("arm", ARMS)
@pytest.mark.parametrize("case", list(ph.CASES))
def test_families_and_class_counts(world, case, arm):
    """what the set-up chose: every smoothed level on the fused block-tridiagonal kernels, levels 1 and 2 in one launch
    each way, a dictionary on every smoothed level (none in `plain`) whose class count is at least the pattern's
    period and at most 32 -- the device's own count, printed beside the host-side proxy's"""
    r = world.ref(case)
    H = world.hier(case, arm)
    lv = H.dictionary_levels()
    proxy = [ph.input_classes(r["Ho"], k)[0] for k in jh.smoothed_levels(r["Ho"])]
    print(f"[periodic] families {case} {arm}: kinds {H.level_kinds()} classes (device) {lv} (proxy) {proxy} elements {r['ne']} "
          f"paired down {[H.paired_levels(s, 'down') for s in (1, 2, 3, 8)]} up {[H.paired_levels(s, 'up') for s in (2, 3, 8)]}")
    assert H.level_kinds() == ["fused_btd"] * 3 + ["coarsest"]
    for nPre, nPost in ph.sweeps_of(case):
        assert H.paired_levels(nPre, "down") == [1] and H.paired_levels(nPost, "up") == [1], (nPre, nPost)
    if arm == "plain":
        assert lv == {}
        return
    assert sorted(lv) == [0, 1, 2], lv
    period = ph.CASES[case][5]
    for k, count in lv.items():
        assert period <= count <= ph.CAP, (case, k, count)
    assert lv == world.hier(case, "lds").dictionary_levels()


# ---- 1. one cycle -----------------------------------------------------------------------------------------------------------
ONE = [(c, s, st) for c in ph.CASES for s in ph.sweeps_of(c) for st in ("x0", "none")]


@pytest.mark.parametrize("case,sweeps,start", ONE, ids=[f"{c}-V{s[0]}{s[1]}-{st}" for c, s, st in ONE])
def test_one_cycle_against_the_oracle(mg, world, case, sweeps, start):
    """every arm against the oracle and with its counters, then the arms against one another as bits; the host-pointer
    entry has vcycle_dev's bits"""
    r = world.ref(case)
    nPre, nPost = sweeps
    b, N = r["b"], r["N"]
    x0 = r["x0"] if start == "x0" else None
    out = {}
    for arm in ARMS:
        H = world.hier(case, arm)
        ctx = H.ctx
        dx, db = ctx.alloc(N), ctx.to_device(b)
        dx0 = None if x0 is None else ctx.to_device(x0)
        before = _counters(ctx)
        H.vcycle_dev(dx0, db, dx, nPre, nPost, ph.ALPHA)
        x = dx.download()
        grown = _grown(ctx, before)
        print(f"[periodic] {case} {arm} V({nPre},{nPost}) {start}: element-thread / records-in-LDS / two-level element-thread / "
              f"replay launches {grown}")
        _assert_rule_1(r, x, r["one"][sweeps, start], b, x0, ph.ONE_CYCLE_ITERATE_TOL, ("one cycle", case, arm, sweeps, start))
        assert grown == _launch_counts(arm, sweeps), (case, arm, sweeps, grown)
        out[arm] = x
    for arm in ARMS[1:]:
        assert _same(out[arm], out["lds"]), (arm, float(np.max(np.abs(out[arm] - out["lds"]))))
    H = world.hier(case, "lds")
    xh = mg.multigrid_v_cycle(H, np.zeros(N) if x0 is None else x0, b, nPre=nPre, nPost=nPost, alpha=ph.ALPHA)
    assert _same(xh, out["lds"]), float(np.max(np.abs(xh - out["lds"])))


# ---- 2. loops ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(ph.CASES))
def test_cycles_back_to_back(world, case):
    """vcycles_dev(k), k = 1, 2, 3: every iterate against the oracle's cycle repeated; three cycles in one call are three
    separate calls bit for bit; the arms agree as bits"""
    r = world.ref(case)
    b, N = r["b"], r["N"]
    out = {}
    for arm in ARMS:
        H = world.hier(case, arm)
        ctx = H.ctx
        bd, z = ctx.to_device(b), ctx.to_device(np.zeros(N))
        dx = ctx.alloc(N)
        before = _counters(ctx)
        for k in (1, 2, 3):
            H.vcycles_dev(z, bd, dx, k, 3, 3, ph.ALPHA)
            x = dx.download()
            _assert_rule_1(r, x, r["xs"][k - 1], b, None, ph.loop_iterate_tol(k), ("loop", case, arm, k))
            rk = float(np.linalg.norm(r["A"] @ x - b))
            assert np.isclose(rk, r["res"][k - 1], rtol=1e-8, atol=1e-11 * max(np.linalg.norm(b), r["res"][0])), (k, rk, r["res"][k - 1])
        grown = _grown(ctx, before)
        print(f"[periodic] {case} {arm} vcycles_dev(1, 2, 3): launches {grown}")
        elem, lds, pair, _ = _launch_counts(arm, (3, 3))
        assert (grown[0] > 0) == (elem > 0) and grown[1] == (grown[0] if lds else 0) and grown[2] == 6 * pair, (arm, grown)
        xa, xb = ctx.to_device(np.zeros(N)), ctx.alloc(N)
        for _ in range(3):
            H.vcycle_dev(xa, bd, xb, 3, 3, ph.ALPHA)
            xa, xb = xb, xa
        assert _same(xa.download(), x), float(np.max(np.abs(xa.download() - x)))
        out[arm] = x
    for arm in ARMS[1:]:
        assert _same(out[arm], out["lds"]), (arm, float(np.max(np.abs(out[arm] - out["lds"]))))


@pytest.mark.parametrize("case", list(ph.CASES))
def test_device_loop_with_checks(mg, world, case):
    """multigrid_dev, the residual test formed inside the fine-level launch: a check after every cycle and after every
    third; the histories against ||A x_k - b|| of the reference, the last iterate against its fourth"""
    r = world.ref(case)
    b, N, ref = r["b"], r["N"], np.asarray(r["res"])
    atol = 1e-11 * max(np.linalg.norm(b), ref[0])
    last = {}
    for arm in ARMS:
        H = world.hier(case, arm)
        ctx = H.ctx
        bd, z = ctx.to_device(b), ctx.to_device(np.zeros(N))
        out = {}
        for every, at in ((1, [0, 1, 2, 3]), (3, [2, 3])):
            before = _counters(ctx)
            dx, ncyc, res = mg.multigrid_dev(H, z, bd, ph.NCYC, 1e-30, check_every=every, nPre=3, nPost=3, alpha=ph.ALPHA)
            print(f"[periodic] {case} {arm} multigrid_dev check_every={every}: {ncyc} cycles, res {res} reference {ref[at].tolist()} "
                  f"launches {_grown(ctx, before)}")
            assert ncyc == ph.NCYC and len(res) == len(at)
            assert np.allclose(res, ref[at], rtol=1e-8, atol=atol)
            out[every] = dx.download()
            _assert_rule_1(r, out[every], r["xs"][-1], b, None, ph.loop_iterate_tol(ph.NCYC), ("device loop", case, arm, every))
        assert _same(out[1], out[3])
        last[arm] = out[1]
    for arm in ARMS[1:]:
        assert _same(last[arm], last["lds"]), (arm, float(np.max(np.abs(last[arm] - last["lds"]))))


# ---- 3. K columns -----------------------------------------------------------------------------------------------------------
def test_k_columns(mg, world):
    """vcycle_multi_dev with K = 3 on distinct columns, records in LDS: every column against the oracle's cycle of that
    column, every column the single-column call bit for bit"""
    case, K = ph.MULTI_CASE, ph.MULTI_K
    r = world.ref(case)
    H = world.hier(case, "lds")
    ctx = H.ctx
    N = r["N"]
    B, X0 = r["B"], r["X0"]
    print(f"[periodic] {case} lds K={K}: multi_info {H.multi_info(K, 3, 3)}")
    X = _multi(mg, H, ctx, X0, B, 3, 3, N + 1)
    for j in range(K):
        _assert_rule_1(r, X[:, j], r["XR"][:, j], B[:, j], X0[:, j], ph.COLUMN_ITERATE_TOL, ("column", case, "lds", K, j))
    before = _counters(ctx)
    R = _single(H, ctx, X0, B, 3, 3)
    assert _grown(ctx, before) == tuple(K * c for c in _launch_counts("lds", (3, 3)))
    for j in range(K):
        assert _same(X[:, j], R[:, j]), (j, float(np.max(np.abs(X[:, j] - R[:, j]))))


# ---- 4. the control ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ("transfer", "operator"))
@pytest.mark.parametrize("level", (0, 1, 2))
def test_the_comparison_sees_a_neighbours_record(mg, oracle, world, level, mutation):
    """the control: a hierarchy that carries the neighbour's transfer block or operator block row at one interior element
    of one level (jitter_helpers) goes to the device with the records in LDS.  Its cycle is the oracle's cycle of that
    hierarchy to the bound -- and misses the unchanged oracle's by 100 times the bound and more: what a kernel reading
    the wrong element's record would compute does not pass test_one_cycle_against_the_oracle.

    The device's smoother takes its blocks from the operator it is given, so the changed operator row goes with the
    inverse of its (the neighbour's) diagonal block in the oracle too (neighbour_inverse_block).

    Which kernels ran is asserted.  With the changed transfer every new kernel runs as in the `lds` arm.  The changed
    operator row is no longer the mirror image of its neighbours' couplings, and the set-up declines the forms that rest
    on that on the level it finds it on: at level 0 the fine level has no dictionary and runs neither element-thread
    kernel, while levels 1 and 2 keep their two-level element-thread launches; at level 1 or 2 those two levels are not
    paired, while the fine level keeps the element-thread kernels with the records in LDS."""
    case = ph.LONG_CASE
    r = world.ref(case)
    Ho, b, x0, N = r["Ho"], r["b"], r["x0"], r["N"]
    ctx = world.ctx("lds")
    with contextlib.ExitStack() as stack:
        stack.enter_context(jh.MUTATIONS[mutation](Ho, level))
        if mutation == "operator":
            stack.enter_context(jh.neighbour_inverse_block(Ho, level))
        xm = oracle.multigrid_v_cycle(Ho, x0, b)
        H = mg.MeshHierarchy.from_reference(Ho, ctx=ctx)
    try:
        lv, paired = H.dictionary_levels(), H.paired_levels()
        assert H.level_kinds() == ["fused_btd"] * 3 + ["coarsest"]
        dx = ctx.alloc(N)
        before = _counters(ctx)
        H.vcycle_dev(ctx.to_device(x0), ctx.to_device(b), dx, 3, 3, ph.ALPHA)
        x = dx.download()
        grown = _grown(ctx, before)
    finally:
        H.free()
    scale = jh.cycle_scale(Ho, b, x0)
    own = float(np.linalg.norm(r["A"] @ (x - xm))) / scale
    other = float(np.linalg.norm(r["A"] @ (x - r["one"][(3, 3), "x0"]))) / scale
    print(f"[periodic] control, {mutation} at level {level}: classes {lv} paired {paired} launches {grown}; against the oracle of "
          f"the changed hierarchy {own:.3e}, of the unchanged one {other:.3e}")
    if mutation == "transfer":
        assert sorted(lv) == [0, 1, 2] and max(lv.values()) <= ph.CAP and paired == [1], (lv, paired)
        assert grown == _launch_counts("lds", (3, 3)), grown
    elif level == 0:
        assert sorted(lv) == [1, 2] and paired == [1] and grown == (0, 0, 2, 0), (lv, paired, grown)
    else:
        assert 0 in lv and paired == [] and grown == (2, 2, 0, 1), (lv, paired, grown)
    assert own <= ph.RESIDUAL_TOL and other >= 100.0 * ph.RESIDUAL_TOL, (own, other)


def test_print_largest_figures():
    """the largest ||A (x - x_ref)|| / scale, and the largest ||x - x_ref|| / ||x_ref|| as a part of its bound, of every
    case and arm, for the record"""
    for key in sorted(FIGURES, key=str):
        print(f"[periodic] largest {key}: residual {FIGURES[key][0]:.3e}   iterate / bound {FIGURES[key][1]:.3f}")
    assert all(v[0] <= ph.RESIDUAL_TOL and v[1] <= 1.0 for v in FIGURES.values())
