"""Agglomeration ratios at which the tile planners (csrc/host_plan.hpp) change regime: ratios other than 2 and 4, where
 * two levels have no common tile and must take one launch each (pair_down_plan / pair_up_plan give own == 0),
 * a checkpoint launch of multigrid() owns less than half a tile (its partial sums were once reserved for more),
 * a single-level fused tile does not exist and the cycle takes the unfused sequence (the set-up keeps a structured
   transfer for ratios up to 64 only: (128, 2) runs the unfused sequence for that reason, (60, 2) and (52, 2) at block
   size 8 for want of a tile),
 * tile boundaries fall on floor((TE - 2 halo) / rho) * rho instead of a divisor of the level size.
Reference: the NumPy / SciPy V-cycle of the oracle (oracle.multigrid_v_cycle, repeated for the loops) on the CSC operators
of UniformDgAggHierarchy through tests/dist_helpers.LocalRef (block-Jacobi blocks by dense LU).  With a first ratio of
28 and more the cycle is a poor method (the reference's own residual grows 4x .. 8x per cycle): these are arithmetic
fixtures, which is why no loop here runs more than 4 cycles.

Tolerances: one cycle ||A (x - x_ref)|| <= 1e-12 (||b|| + ||A x0||) as tests/test_gpu_random_shapes.py (reference against
reference -- sparse LU against dense LU coarsest solve -- on these inputs: at most 5.4e-15 of that scale); residual
histories rtol 1e-8, atol 1e-11 max(||b||, res[0]) as tests/test_gpu_solvers.py::test_multigrid_device_loop (reference
against reference over 5 cycles: 2.9e-12 relative); the same arithmetic in another launch split rtol 1e-10."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (n, p, pAgg, ratios, (nPre, nPost))
CASES = {
    "pair_16_16": (8192, 3, 1, (4, 16, 16), (3, 3)),      # the descent of levels 1, 2 has no two-level tile
    "pair_16_8": (8192, 3, 1, (4, 16, 8), (3, 3)),        # the same, unequal ratios
    "pair_32_2": (5120, 3, 1, (2, 32, 2), (3, 3)),        # te_b < 2 (nPre + 1): the plan's numerator is negative
    "pair_13_13": (5408, 1, 1, (4, 13, 13), (3, 3)),      # the first equal ratio without a tile; block size 2 fine level
    "pair_12_2_v88": (4608, 3, 1, (4, 12, 2), (8, 8)),    # a tile at 3 sweeps, none at 8
    "chk_60": (7680, 3, 1, (60, 2), (3, 3)),              # the launch between two cycles owns one agglomerate < TE / 2
    "chk_62_b2": (7440, 1, 1, (62, 2), (4, 3)),           # the same at block size 2, halo 8
    "chk_28_b8": (5600, 7, 1, (28, 2), (3, 3)),           # the same at block size 8
    "mid_52_b8": (5200, 7, 1, (52, 2), (3, 3)),           # one cycle fused, the launch between two cycles has no tile
    "none_128": (6144, 3, 1, (128, 2), (3, 3)),           # a ratio above 64: no structured transfer, the unfused sequence
    "none_60_b8": (5760, 7, 1, (60, 2), (3, 3)),          # block size 8: the fused descent itself has no tile (64 - 8 < 60)
    "odd_7_3_5": (3885, 3, 1, (7, 3, 5), (3, 3)),         # odd ratios, n a multiple of no tile
    "odd_3_3_3_p0": (3888, 2, 0, (3, 3, 3), (2, 2)),      # one coarse row per agglomerate, odd ratios
}
NO_PAIR_DOWN = ("pair_16_16", "pair_16_8", "pair_32_2", "pair_13_13", "pair_12_2_v88")
OWNED_BELOW_HALF = ("chk_60", "chk_62_b2", "chk_28_b8")
ALPHA = 2.0 / 3.0
NCYC = 4


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    return mg.Context(0)


class _Built:
    """reference operators, reference cycles and the device hierarchy of a case, each made once per module"""

    def __init__(self, o, mg, ctx):
        self.o, self.mg, self.ctx = o, mg, ctx
        self.cases, self.hiers, self.build_s = {}, {}, {}

    def case(self, name):
        if name not in self.cases:
            from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
            from dist_helpers import LocalRef
            n, p, pAgg, ratios, (nPre, nPost) = CASES[name]
            t0 = time.perf_counter()
            U = UniformDgAggHierarchy(n, p=p, pAgg=pAgg, ratios=ratios)
            Ho = LocalRef(self.o, U)
            b = U.rhs()
            # the reference loop from a zero guess: iterates and residual norms of NCYC cycles (src/solvers.jl:124-127)
            A = Ho.mStiffness[0]
            xs, res = [], []
            x = np.zeros(len(b))
            for _ in range(NCYC):
                x = self.o.multigrid_v_cycle(Ho, x, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
                xs.append(x)
                res.append(float(np.linalg.norm(A @ x - b)))
            self.build_s[name] = time.perf_counter() - t0
            print(f"[ratio_regimes] {name}: reference build + {NCYC} cycles {self.build_s[name]:.2f} s, res {res}")
            self.cases[name] = dict(U=U, Ho=Ho, b=b, A=A, xs=xs, res=res, nPre=nPre, nPost=nPost)
        return self.cases[name]

    def hier(self, name):
        """the benchmark's route: build_device_hierarchy, host copies released"""
        if name not in self.hiers:
            from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
            c = self.case(name)
            self.hiers[name] = build_device_hierarchy(c["U"], self.ctx, csc=(c["Ho"].mStiffness, c["Ho"].mInterpolation))
        return self.hiers[name]

    def close(self):
        for H in self.hiers.values():
            H.free()


@pytest.fixture(scope="module")
def built(oracle, mg, ctx):
    B = _Built(oracle, mg, ctx)
    yield B
    B.close()


def _assert_cycle(c, x, xr, x0):
    A, b = c["A"], c["b"]
    scale = np.linalg.norm(b) + (np.linalg.norm(A @ x0) if x0 is not None else 0.0)
    d = float(np.linalg.norm(A @ (x - xr)))
    print(f"[ratio_regimes] ||A (x - x_ref)|| / scale = {d / scale:.3e}")
    assert np.all(np.isfinite(x)) and d <= 1e-12 * scale, (d, scale)


def _assert_history(c, res, ref):
    res, ref = np.asarray(res), np.asarray(ref)
    print(f"[ratio_regimes] residual history {res.tolist()} reference {ref.tolist()}")
    assert res.shape == ref.shape
    assert np.allclose(res, ref, rtol=1e-8, atol=1e-11 * max(np.linalg.norm(c["b"]), ref[0]))


def _explicit_hierarchy(mg, ctx, c, keep_host):
    """descriptors, operators, smoothers and transfers handed over one by one (as tests/test_gpu_blockgs.py)"""
    from agglomerationmultigrid1d_amd import _lib
    U, Ho = c["U"], c["Ho"]
    nl = U.nlevels
    ops = [mg.DeviceOperator(Ho.mStiffness[k], _lib.OP_STIFFNESS, ctx) for k in range(nl)]
    Ls = [mg.DeviceOperator(Ho.mInterpolation[k], _lib.OP_TRANSFER, ctx) for k in range(nl - 1)]
    desc = [U.descriptor(k) for k in range(nl)]
    sms = [mg.BlockJacobi(ops[k], desc[k].mBlockInds, ctx) for k in range(nl - 1)]
    return mg.MeshHierarchy(desc, ops, sms, Ls, ctx=ctx, keep_host=keep_host)


@pytest.mark.parametrize("name", list(CASES))
def test_one_cycle_against_the_reference(oracle, mg, built, name):
    c = built.case(name)
    H = built.hier(name)
    assert all(H.structured_levels()), H.level_kinds()
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    x0 = oracle.splitmix_normal(len(b), 11)
    xr = oracle.multigrid_v_cycle(c["Ho"], x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    x = mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    _assert_cycle(c, x, xr, x0)
    # zero initial guess: no vector (what ldiv! uses) and a vector of zeros
    xz = mg.multigrid_v_cycle(H, None, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    _assert_cycle(c, xz, c["xs"][0], None)
    xz0 = mg.multigrid_v_cycle(H, np.zeros(len(b)), b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    _assert_cycle(c, xz0, c["xs"][0], None)


@pytest.mark.parametrize("keep_host", [True, False])
@pytest.mark.parametrize("name", ["pair_16_16", "none_128", "mid_52_b8", "none_60_b8"])
def test_explicit_route_against_the_reference(oracle, mg, ctx, built, name, keep_host):
    """the hierarchy built from operators, smoothers and transfers handed over one by one; the unfused sequence forms
    CSR copies of the operators on the way, with the host copies kept and released"""
    c = built.case(name)
    H = _explicit_hierarchy(mg, ctx, c, keep_host)
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    x0 = oracle.splitmix_normal(len(b), 12)
    xr = oracle.multigrid_v_cycle(c["Ho"], x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    _assert_cycle(c, mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA), xr, x0)
    _assert_cycle(c, mg.multigrid_v_cycle(H, None, b, nPre=nPre, nPost=nPost, alpha=ALPHA), c["xs"][0], None)
    x, it, res, _ = mg.multigrid(H, np.zeros(len(b)), b, NCYC, 0.0, exact=False, nPre=nPre, nPost=nPost, alpha=ALPHA)
    assert it == NCYC
    _assert_history(c, res, c["res"])
    # the same bits as the benchmark's route
    xb = mg.multigrid(built.hier(name), np.zeros(len(b)), b, NCYC, 0.0, exact=False, nPre=nPre, nPost=nPost, alpha=ALPHA)[0]
    assert np.array_equal(x, xb)
    H.free()


@pytest.mark.parametrize("name", list(CASES))
def test_cycle_loops_against_the_reference(mg, ctx, built, name):
    c = built.case(name)
    H = built.hier(name)
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    N = len(b)
    nb = np.linalg.norm(b)
    # three cycles back to back (between two cycles the fine level takes one fused launch where that launch has a tile)
    dx = ctx.alloc(N)
    H.vcycles_dev(ctx.to_device(np.zeros(N)), ctx.to_device(b), dx, 3, nPre, nPost, ALPHA)
    x3 = dx.download()
    r3 = float(np.linalg.norm(c["A"] @ x3 - b))
    print(f"[ratio_regimes] vcycles_dev(3): residual {r3} reference {c['res'][2]}")
    assert np.all(np.isfinite(x3))
    assert np.isclose(r3, c["res"][2], rtol=1e-8, atol=1e-11 * max(nb, c["res"][0]))
    # multigrid(): the loop with the residual test of every cycle
    x, it, res, err = mg.multigrid(H, np.zeros(N), b, NCYC, 0.0, exact=False, nPre=nPre, nPost=nPost, alpha=ALPHA)
    assert it == NCYC and err == []
    _assert_history(c, res, c["res"])
    # its third iterate and the three cycles back to back: the same arithmetic
    x3m = mg.multigrid(H, np.zeros(N), b, 3, 0.0, exact=False, nPre=nPre, nPost=nPost, alpha=ALPHA)[0]
    assert np.array_equal(x3m, x3)
    assert np.all(np.isfinite(x))


@pytest.mark.parametrize("name", list(CASES))
def test_checkpoints_inside_the_launch_and_apart(mg, ctx, built, name):
    """AGGMG_OPT_MG_CHECKPOINT 1 (residual test formed inside the fine-level launch) and 0 (a residual launch per check)"""
    from agglomerationmultigrid1d_amd import _lib
    c = built.case(name)
    H = built.hier(name)
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    z = np.zeros(len(b))
    exact = name == "chk_60"     # both sums of a checkpoint are read
    kw = dict(nPre=nPre, nPost=nPost, alpha=ALPHA)
    out = {}
    was = ctx.option(_lib.OPT_MG_CHECKPOINT, 1)
    try:
        for on in (1, 0):
            ctx.set_option(_lib.OPT_MG_CHECKPOINT, on)
            out[on] = (mg.multigrid(H, z, b, NCYC, 0.0, exact=exact, **kw), mg.multigrid(H, z, b, NCYC, 0.0, exact=False, check_every=2, **kw))
    finally:
        ctx.set_option(_lib.OPT_MG_CHECKPOINT, was)
    (x1, it1, res1, err1), (x1c, it1c, res1c, _) = out[1]
    (x0, it0, res0, err0), (x0c, it0c, res0c, _) = out[0]
    print(f"[ratio_regimes] checkpoint on {res1} off {res0}; every 2nd: on {res1c} off {res0c}; err on {err1} off {err0}")
    assert it1 == it0 == NCYC and it1c == it0c == NCYC and len(res1c) == len(res0c) == NCYC // 2
    assert np.allclose(res1, res0, rtol=1e-10) and np.allclose(res1c, res0c, rtol=1e-10)
    assert np.allclose(res1c, res1[1::2], rtol=1e-10)
    _assert_history(c, res1, c["res"])
    _assert_history(c, res0, c["res"])
    if exact:
        assert len(err1) == len(err0) == NCYC and np.all(np.isfinite(err1))
        assert np.allclose(err1, err0, rtol=1e-8, atol=1e-11)     # (tests/test_gpu_solvers.py: the same pair of forms)
    # the same iterates bit for bit, as on the ratios tests/test_gpu_solvers.py runs
    assert np.array_equal(x1, x0) and np.array_equal(x1c, x0c) and np.array_equal(x1, x1c)


def _launch_counts(ctx, run):
    run()                      # work space allocated outside the profiled call
    ctx.synchronize()
    ctx.profile_enable(True)
    try:
        run()
        return ctx.profile_collect()
    finally:
        ctx.profile_enable(False)


def _assert_counts_follow_the_report(H, ctx, nPre, nPost, b):
    """one V-cycle: a level the reports call unpaired runs launches of its own each way -- one fused launch, or (more
    sweeps than a fused launch holds: V(8,8) descents with their residual) the unfused sequence with its residual /
    prolongation launch -- and the second level of a reported pair runs none"""
    db, dx = ctx.to_device(b), ctx.alloc(len(b))
    stats = _launch_counts(ctx, lambda: H.vcycle_dev(None, db, dx, nPre, nPost, ALPHA))
    for kind, apart, direction, ns in (("fused_down", "residual", "down", nPre), ("fused_up", "prolong", "up", nPost)):
        paired = H.paired_levels(ns, direction)
        for k in range(H.nlevels - 1):
            fused = stats.get((kind, k), (0.0, 0))[1]
            unfused = stats.get((apart, k), (0.0, 0))[1]
            if (k - 1) in paired:
                assert fused == 0 and unfused == 0, (kind, k, paired, stats)
            else:
                assert (fused, unfused) in ((1, 0), (0, 1)), (kind, k, paired, stats)
            if k in paired:
                assert (fused, unfused) == (1, 0), (kind, k, paired, stats)
    return stats


@pytest.mark.parametrize("name", NO_PAIR_DOWN)
def test_pairing_reports_are_truthful(mg, ctx, built, name):
    c = built.case(name)
    H = built.hier(name)
    nPre, nPost = c["nPre"], c["nPost"]
    assert H.paired_levels(nPre) == [], "the report names a two-level descent that has no tile"
    if name == "pair_12_2_v88":
        assert H.paired_levels(3) == [1]      # the same levels at three sweeps have one
    _assert_counts_follow_the_report(H, ctx, nPre, nPost, c["b"])
    assert H.nlevels == 4 and all(k == "fused_btd" for k in H.level_kinds()[:-1])


def test_pairing_control_case(mg, ctx):
    """ratios (4, 8, 8): a two-level tile exists both ways, levels 1 and 2 share their launches"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(4096, p=3, pAgg=1, ratios=(4, 8, 8))
    H = build_device_hierarchy(U, ctx)
    assert H.paired_levels(3) == [1] and H.paired_levels(3, "up") == [1]
    stats = _assert_counts_follow_the_report(H, ctx, 3, 3, U.rhs())
    assert stats[("fused_down", 1)][1] == 1 and ("fused_down", 2) not in stats and ("fused_up", 2) not in stats
    H.free()


# K columns --------------------------------------------------------------------------------------------------------
from test_gpu_multi_rhs import _assert_columns_equal, _multi, _single  # noqa: E402

K_CASES = {"odd_7_3_5": True, "pair_16_16": None, "chk_60": False, "none_128": False}   # K-column launches? (None: either)


@pytest.mark.parametrize("name", list(K_CASES))
def test_k_columns(oracle, mg, ctx, built, name):
    c = built.case(name)
    H = built.hier(name)
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    N = len(b)
    rng = np.random.default_rng(5)
    B = rng.standard_normal((N, 8)) * np.linalg.norm(b) / np.sqrt(N)
    B[:, 0] = b
    X0 = rng.standard_normal((N, 8))
    x0 = X0[:, 0].copy()
    xr = oracle.multigrid_v_cycle(c["Ho"], x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
    for K in (3, 8):
        fused, group = H.multi_info(K, nPre, nPost)
        if K_CASES[name] is not None:
            assert fused == K_CASES[name], (name, K, fused, group)
        assert (1 <= group <= K) if fused else group == 1
        # the report against the launches: one fused descent of the fine level per group of columns
        dB, dX = mg.DeviceMatrix(ctx, N, K), mg.DeviceMatrix(ctx, N, K)
        dB.upload(np.asfortranarray(B[:, :K]))
        stats = _launch_counts(ctx, lambda: H.vcycle_multi_dev(None, dB, dX, nPre=nPre, nPost=nPost))
        if name != "none_128":     # (no fused fine-level launch there at all)
            assert stats.get(("fused_down", 0), (0.0, 0))[1] == (-(-K // group) if fused else K), (fused, group, stats)
        for guess in (X0, None):
            R = _single(H, ctx, None if guess is None else guess[:, :K], B[:, :K], nPre, nPost)
            X = _multi(mg, H, ctx, None if guess is None else guess[:, :K], B[:, :K], nPre, nPost, N + (K % 2))
            _assert_columns_equal(X, R)
            if guess is None:
                _assert_cycle(c, X[:, 0], c["xs"][0], None)
            else:
                _assert_cycle(c, X[:, 0], xr, x0)


@pytest.mark.parametrize("name", ["odd_7_3_5", "chk_60"])
def test_symmetric_residual_on_and_off(oracle, mg, built, name):
    """AGGMG_OPT_SYMMETRIC_RESIDUAL: the lossless symmetric form of the residual's entries gives the same bits"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    c = built.case(name)
    nPre, nPost, b = c["nPre"], c["nPost"], c["b"]
    x0 = oracle.splitmix_normal(len(b), 13)
    out, levels = {}, {}
    for on in (1, 0):
        cx = mg.Context(0)
        cx.set_option(_lib.OPT_SYMMETRIC_RESIDUAL, on)
        H = build_device_hierarchy(c["U"], cx, csc=(c["Ho"].mStiffness, c["Ho"].mInterpolation))
        levels[on] = H.sym_residual_levels()
        x = mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA)
        xm = mg.multigrid(H, np.zeros(len(b)), b, 3, 0.0, exact=False, nPre=nPre, nPost=nPost, alpha=ALPHA)
        out[on] = (x, xm[0], xm[2])
        H.free()
    assert levels[1] and not levels[0], levels
    assert np.array_equal(out[1][0], out[0][0]) and np.array_equal(out[1][1], out[0][1]) and out[1][2] == out[0][2]
    _assert_cycle(c, out[1][0], oracle.multigrid_v_cycle(c["Ho"], x0, b, nPre=nPre, nPost=nPost, alpha=ALPHA), x0)
