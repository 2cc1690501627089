"""The K-column launches of a dictionary level on the element-thread layout (csrc/multi_elem_kernels.hpp,
btd_elem_rec_multi_kernel; AGGMG_OPT_MULTI_ELEMENT_THREADS): one thread per element, the class records
in LDS, the columns of a group walked by the workgroup.  Every column must be BIT FOR BIT what the K-column cycle gives with
the option off (btd_multi_kernel, arm B) and what the single-column cycle gives on that column (vcycle_dev, replaying its
pre-smoothing by default, arm C), compared as 64-bit patterns.  Arm A (option on) must have launched the new kernel
exactly twice per group of 8 columns and cycle -- level 0 is the only level with blocks of 4 rows on these hierarchies --
and arms B and C not at all; the counters of the single-column element-thread kernels must not move differently.

What can go wrong is a wrong column stride, plane, class record, mask, barrier or rounding, so the shapes are the smallest
that put one or two tiles (n = 256), five with a ragged last one (n = 1024) and a table at the cap (n = 36, 32 classes) under
the kernel, with agglomerates of 4 and of 2, both orders of the boundary conditions, and one operator on unequal elements
(tests/periodic_helpers.py, "p3_512": a period of 3 widths, a level-0 dictionary of at most 32 classes that vary inside a
tile).  K = 1 .. 11 covers a full group, a group and a remainder, and remainders that do not fill a pass; the leading
dimension N + 3 puts the columns on odd multiples of 8 bytes.  The pad rows of X and a guard column on either side carry a
NaN pattern that must come back unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)
KS = (1, 2, 3, 5, 8, 9, 11)
KMAX = max(KS)
GROUP = 8                                  # columns of a launch (aggmg_hier_multi_info)
POISON = np.uint64(0x7FF8DEADBEEF0123)     # a quiet NaN with a payload


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


class _Arm:
    """a context with AGGMG_OPT_MULTI_ELEMENT_THREADS set one way, and its hierarchies by case"""

    def __init__(self, mg, on, **options):
        from agglomerationmultigrid1d_amd import _lib
        self.ctx = mg.Context(0)
        self.ctx.set_option(_lib.OPT_MULTI_ELEMENT_THREADS, on)
        for name, value in options.items():
            self.ctx.set_option(getattr(_lib, name), value)
        self.hiers = {}

    def hier(self, key, make):
        if key not in self.hiers:
            self.hiers[key] = make(self.ctx)
        return self.hiers[key]

    def counters(self):
        c = self.ctx
        return np.array([c.multi_element_thread_launches(), c.element_thread_launches(), c.element_record_lds_launches(),
                         c.replay_launches()])

    def close(self):
        for H in self.hiers.values():
            H.free()
        self.hiers = {}
        self.ctx.close()


@pytest.fixture(scope="module")
def arms(mg):
    a = {"on": _Arm(mg, 1), "off": _Arm(mg, 0)}
    yield a
    for arm in a.values():
        arm.close()


def _uniform(n, ratios, bc=None, **kw):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=ratios, bc=bc)
    return lambda ctx: build_device_hierarchy(U, ctx, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _padded(ctx, A, ld):
    """A (N, K) -> a device buffer of K + 2 columns of ld doubles, A in columns 1 .. K, the poison everywhere else; and the
    pointer of column 1"""
    N, K = A.shape
    buf = np.full((ld, K + 2), POISON, dtype=np.uint64, order="F").view(np.float64)
    buf[:N, 1:K + 1] = A
    d = ctx.to_device(buf.ravel(order="F"))
    return d, d.ptr.value + 8 * ld


def _multi(arm, H, X0, B, npre, npost, ld, ncyc=1):
    """ncyc K-column cycles, the output feeding the next first iterate -> (X, the counters' growth); the poison of the pad rows
    and guard columns of X checked after every cycle"""
    ctx = arm.ctx
    N, K = B.shape
    dB, pB = _padded(ctx, B, ld)
    src = None
    if X0 is not None:
        dX0, src = _padded(ctx, X0, ld)
    outs = [_padded(ctx, np.full((N, K), np.nan), ld) for _ in range(2)]
    k0 = arm.counters()
    for c in range(ncyc):
        dX, pX = outs[c % 2]
        H.vcycle_multi_dev(src, pB, pX, K, ld, npre, npost)
        got = dX.download().reshape((ld, K + 2), order="F")
        assert np.all(_bits(got[:, 0]) == POISON) and np.all(_bits(got[:, K + 1]) == POISON), "a guard column was written"
        assert np.all(_bits(got[N:, :]) == POISON), "a pad row was written"
        src = pX
    return np.array(got[:N, 1:K + 1], order="F"), arm.counters() - k0


def _single(arm, H, X0, B, npre, npost, ncyc=1):
    """column by column through vcycle_dev on slices of one device matrix -> (X, the counters' growth)"""
    ctx = arm.ctx
    N, K = B.shape
    dB = ctx.to_device(np.asfortranarray(B).ravel(order="F"))
    dX0 = None if X0 is None else ctx.to_device(np.asfortranarray(X0).ravel(order="F"))
    xs = [ctx.alloc(N), ctx.alloc(N)]
    out = np.empty((N, K), order="F")
    k0 = arm.counters()
    for j in range(K):
        src = None if dX0 is None else dX0.ptr.value + 8 * j * N
        for c in range(ncyc):
            H.vcycle_dev(src, dB.ptr.value + 8 * j * N, xs[c % 2], npre, npost)
            src = xs[c % 2]
        out[:, j] = xs[(ncyc - 1) % 2].download()
    return out, arm.counters() - k0


def _ngroups(K):
    return -(-K // GROUP)


def _three_arms(arms, key, make, sweeps, guesses=(True, False), ks=KS, ncyc=1, weights=None, served=(True, True), seed=0,
                fused=True):
    """arm C once for KMAX columns per (sweeps, guess), then arms A and B for every K: bits, counters, poison.  served: the
    halves of level 0 the new kernel must serve; fused: does the K-column cycle run in column groups at all?"""
    Ha, Hb = arms["on"].hier(key, make), arms["off"].hier(key, make)
    if weights is not None:
        for H in (Ha, Hb):
            H.set_sweep_weights(0, weights[0], weights[1])
    N = Ha._ops[0].shape[0]
    rng = np.random.default_rng(1000 + seed)
    B = rng.standard_normal((N, KMAX))
    G = rng.standard_normal((N, KMAX))
    halves = int(served[0]) + int(served[1])
    for npre, npost in sweeps:
        for K in ks:
            assert Ha.multi_info(K, npre, npost) == ((True, min(K, GROUP)) if fused else (False, 1)), (K, Ha.multi_info(K, npre, npost))
        want_levels = {0: served} if halves else {}
        assert Ha.multi_element_thread_levels(npre, npost) == want_levels, Ha.multi_element_thread_levels(npre, npost)
        assert Hb.multi_element_thread_levels(npre, npost) == {}
        for guess in guesses:
            X0 = G if guess else None
            R, kc = _single(arms["off"], Hb, X0, B, npre, npost, ncyc)
            assert kc[0] == 0, "the single-column cycle counted a K-column element-thread launch"
            assert np.all(np.isfinite(R)) and np.any(R != 0.0)
            for i, K in enumerate(ks):
                ld = N if i % 2 == 0 else N + 3
                x0 = None if X0 is None else X0[:, :K]
                Xa, ka = _multi(arms["on"], Ha, x0, B[:, :K], npre, npost, ld, ncyc)
                Xb, kb = _multi(arms["off"], Hb, x0, B[:, :K], npre, npost, ld, ncyc)
                assert ka[0] == halves * _ngroups(K) * ncyc, (K, ka, halves)
                assert kb[0] == 0 and np.array_equal(ka[1:], kb[1:]), (K, ka, kb)
                for j in range(K):
                    assert _same(Xa[:, j], Xb[:, j]), ("on / off", npre, npost, guess, K, ld, j, float(np.max(np.abs(Xa[:, j] - Xb[:, j]))))
                    assert _same(Xa[:, j], R[:, j]), ("on / single", npre, npost, guess, K, ld, j, float(np.max(np.abs(Xa[:, j] - R[:, j]))))
    return Ha


CASES = {
    "n256_r422": (256, (4, 2, 2), None),
    "n1024_r422": (1024, (4, 2, 2), None),
    "n36_r4": (36, (4,), None),                # 32 classes: the table at the cap, a second round of its loads
    "n256_r222": (256, (2, 2, 2), None),
    "n1024_r222_dirneu": (1024, (2, 2, 2), DIR_NEU),
    "n256_r422_dirneu": (256, (4, 2, 2), DIR_NEU),
}


def _case(name):
    n, ratios, bc = CASES[name]
    return name, _uniform(n, ratios, bc)


def test_option_counter_and_query_exist(mg):
    from agglomerationmultigrid1d_amd import _lib
    assert _lib.OPT_MULTI_ELEMENT_THREADS == 16
    ctx = mg.Context(0)
    try:
        for v in (0, 1):
            ctx.set_option(_lib.OPT_MULTI_ELEMENT_THREADS, v)
        assert ctx.multi_element_thread_launches() == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("case", list(CASES))
def test_v33_every_k_bitwise(arms, case):
    """V(3,3), no first iterate and a random one, every K, ld = N and N + 3"""
    key, make = _case(case)
    H = _three_arms(arms, key, make, ((3, 3),), seed=len(case))
    lv = H.dictionary_levels()
    assert 0 in lv and lv[0] <= 32, lv
    if case == "n36_r4":
        assert lv[0] == 32
    elif case in ("n256_r422", "n1024_r422"):
        assert lv[0] == 7


@pytest.mark.parametrize("case", ["n256_r422", "n1024_r222_dirneu", "n36_r4"])
@pytest.mark.parametrize("sweeps", [(1, 2), (7, 8)])
def test_other_sweep_counts_bitwise(arms, case, sweeps):
    """the smallest halos, and V(7,8): the most sweeps one launch takes -- 7 and the residual in the descent, 8 in the ascent
    (tiles of 240 owned elements)"""
    key, make = _case(case)
    _three_arms(arms, key, make, (sweeps,), seed=sweeps[0])


@pytest.mark.parametrize("case", ["n256_r422", "n1024_r222_dirneu", "n36_r4"])
def test_v88_bitwise(arms, case):
    """V(8,8): eight sweeps and the residual are one more than a descent launch of any fused block-tridiagonal kernel takes
    (btd_launch_ok: sweeps + residual <= 8), so the K-column cycle has no column groups there (aggmg_hier_multi_info) and
    runs the single-column cycle on every column, as before: the same bits in all three arms, no launch of the new kernel"""
    key, make = _case(case)
    _three_arms(arms, key, make, ((8, 8),), served=(False, False), fused=False, seed=8)


def test_unequal_sweep_weights_bitwise(arms):
    """every sweep of a launch has its own weight (wts.w[sw]), the same for every column"""
    n, ratios, bc = CASES["n1024_r422"]
    _three_arms(arms, "n1024_r422_weights", _uniform(n, ratios, bc), ((3, 3),), ks=(3, 8, 11),
                weights=(np.array([0.9, 0.5, 0.7]), np.array([0.3, 0.8, 0.6])), seed=3)


@pytest.mark.parametrize("case", ["n1024_r422", "n256_r222"])
def test_three_cycles_in_sequence_bitwise(arms, case):
    """three cycles, the output feeding the next first iterate"""
    key, make = _case(case)
    _three_arms(arms, key, make, ((3, 3),), ks=(2, 9), ncyc=3, seed=9)


def test_periodic_unequal_elements_bitwise(mg, arms, oracle):
    """"p3_512" of tests/periodic_helpers.py: elements of three widths in turn, so the classes vary inside every tile; its
    level-0 dictionary has at most 32 classes and level 0 is its only level with blocks of 4 rows"""
    import periodic_helpers as ph
    Ho, _ = ph.build(oracle, "p3_512")
    H = _three_arms(arms, "periodic_p3_512", lambda ctx: mg.MeshHierarchy.from_reference(Ho, ctx=ctx), ((3, 3), (1, 2)),
                    ks=(3, 8, 11), seed=5)
    lv = H.dictionary_levels()
    assert 3 <= lv[0] <= 32, lv


# ---- fall-backs: today's kernel, today's bits, the counter still ---------------------------------------------------------
def test_over_the_class_cap_keeps_the_row_kernel(arms):
    """n = 300: more than 32 classes on level 0"""
    H = _three_arms(arms, "n300_r4", _uniform(300, (4,)), ((3, 3),), ks=(3, 11), served=(False, False), seed=30)
    assert H.dictionary_levels()[0] > 32


@pytest.mark.parametrize("sweeps,served", [((0, 3), (False, True)), ((3, 0), (True, False)), ((0, 0), (False, False))])
def test_half_without_sweeps_keeps_the_row_kernel(arms, sweeps, served):
    """a half with no sweep stays on btd_multi_kernel; the other half is served, and the counter says so"""
    key, make = _case("n256_r422")
    _three_arms(arms, key, make, (sweeps,), ks=(3, 9), served=served, seed=sum(sweeps))


@pytest.mark.parametrize("option", ["OPT_ELEMENT_THREADS", "OPT_ELEMENT_RECORDS_LDS", "OPT_OPERATOR_DICTIONARY"])
def test_switched_off_beneath_keeps_the_row_kernel(mg, option):
    """the layout, the records in LDS or the dictionary switched off: no K-column element-thread launch either"""
    a = {"on": _Arm(mg, 1, **{option: 0}), "off": _Arm(mg, 0, **{option: 0})}
    try:
        key, make = _case("n256_r422")
        _three_arms(a, key, make, ((3, 3),), ks=(3, 9), served=(False, False), seed=17)
    finally:
        for arm in a.values():
            arm.close()


def test_patch_levels_zero_sweep_launches_do_not_count(mg):
    """a patchGS0 hierarchy under AGGMG_OPT_PATCH_MULTI: its K-column transfers are zero-sweep launches of btd_multi_kernel
    on the smoother's element blocks, which must not reach the new kernel"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(256, p=3, pAgg=1, ratios=(4, 2, 2))
    a = {"on": _Arm(mg, 1, OPT_PATCH_MULTI=1), "off": _Arm(mg, 0, OPT_PATCH_MULTI=1)}
    try:
        make = lambda ctx: build_device_hierarchy(U, ctx, smoother="patchGS0")   # noqa: E731
        before = a["on"].ctx.patch_multi_launches()
        _three_arms(a, "patchGS0", make, ((2, 1),), ks=(3, 9), served=(False, False), seed=21)
        assert a["on"].ctx.patch_multi_launches() > before, "the K-column patch kernel did not run"
        assert a["on"].ctx.multi_element_thread_launches() == 0
    finally:
        for arm in a.values():
            arm.close()


# ---- through the solvers ----------------------------------------------------------------------------------------------------
def _solver_inputs(H):
    N = H._ops[0].shape[0]
    rng = np.random.default_rng(77)
    return np.asfortranarray(rng.standard_normal((N, 3))), np.asfortranarray(rng.standard_normal((N, 3)))


def _assert_history(got, ref, j):
    assert len(got) == len(ref) and _same(np.array(got, dtype=np.float64), np.array(ref, dtype=np.float64)), (j, got, ref)


def test_pcg_on_a_matrix_bitwise(mg, arms):
    key, make = _case("n256_r422")
    arm = arms["on"]
    H = arm.hier(key, make)
    B, X0 = _solver_inputs(H)
    k0 = arm.ctx.multi_element_thread_launches()
    X, its, res = mg.pcg(H, B, X0, maxiter=30, tol=1e-10)
    assert arm.ctx.multi_element_thread_launches() > k0
    for j in range(3):
        x, it, r = mg.pcg(H, B[:, j].copy(), X0[:, j].copy(), maxiter=30, tol=1e-10)
        assert it > 0 and int(its[j]) == it and _same(X[:, j], x), j
        _assert_history(res[j], r, j)


def test_multigrid_on_a_matrix_bitwise(mg, arms):
    """the histories of multigrid on a matrix are bit for bit those of the single-vector loop in its AGGMG_OPT_MG_CHECKPOINT
    = 0 form, which takes ||A x - b|| from a residual launch of its own as the K-column loop does
    (tests/test_gpu_multi_solve.py); the default form, which sums inside the fine-level launch, gives the same iterates
    and counts"""
    from agglomerationmultigrid1d_amd import _lib
    key, make = _case("n256_r422")
    arm = arms["on"]
    H = arm.hier(key, make)
    B, X0 = _solver_inputs(H)
    k0 = arm.ctx.multi_element_thread_launches()
    X, its, res, err = mg.multigrid(H, X0, B, 12, 1e-9, exact=False)
    assert arm.ctx.multi_element_thread_launches() > k0
    plain = _Arm(mg, 1, OPT_MG_CHECKPOINT=0)
    try:
        H0 = plain.hier(key, make)
        for j in range(3):
            x, it, r, _ = mg.multigrid(H0, X0[:, j].copy(), B[:, j].copy(), 12, 1e-9, exact=False)
            assert it > 0 and int(its[j]) == it and _same(X[:, j], x), j
            _assert_history(res[j], r, j)
            xc, itc, _, _ = mg.multigrid(H, X0[:, j].copy(), B[:, j].copy(), 12, 1e-9, exact=False)
            assert itc == it and _same(X[:, j], xc), j
    finally:
        plain.close()


def test_fgmres_multi_bitwise(mg, arms):
    key, make = _case("n256_r422")
    arm = arms["on"]
    H = arm.hier(key, make)
    B, X0 = _solver_inputs(H)
    kw = dict(restart=8, maxiter=20, tol=1e-10, nPre=2, nPost=1)
    k0 = arm.ctx.multi_element_thread_launches()
    X, its, res = mg.fgmres_multi(H, B, X0=X0, **kw)
    assert arm.ctx.multi_element_thread_launches() > k0
    for j in range(3):
        x, it, r = mg.fgmres(H, B[:, j].copy(), x0=X0[:, j].copy(), **kw)
        assert it > 0 and int(its[j]) == it and _same(X[:, j], x), j
        _assert_history(res[j], r, j)
