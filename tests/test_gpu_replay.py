"""The replayed V-cycle (csrc/elem_kernels.hpp, btd_elem_replay_up_kernel; AGGMG_OPT_REPLAY_PRESMOOTH): the fine level's
descent stores no pre-smoothed iterate, and the ascent rebuilds it -- it reads the cycle's first iterate, runs the
pre-sweeps, adds the prolongation and goes on with the post-sweeps.  The same arithmetic on the same inputs in the same
order, so every result must equal BIT FOR BIT the storing cycle's (option off) and the plain kernels' (dictionary off),
compared as 64-bit patterns.  Three arms per case, each running vcycle_dev three times, ping-ponging x; the replay counter
(aggmg_replay_launches) is asserted exactly: one per cycle that replays, 0 in the other two arms and in every fallback.

What can go wrong is a wrong element, mask, weight or rounding at a tile's or the level's end, or a stale vector, so the
shapes are the smallest that put those ends everywhere: at V(3,3) the replaying ascent owns 256 - 2 * 6 = 244 elements of
a 256-element tile and the descent 248, with n at, one agglomerate past and on either side of their multiples."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RATIOS = (4, 2, 2)
DIR_NEU = (("dir", 1.0), ("neu", -0.25))   # Dirichlet left / Neumann right (the default is the other way round)
TILE = 256                                  # elements of an element-thread tile (kElemThreads)
NCYC = 3


def _owned(halo, align):
    """host_plan.hpp fused_tile_plan(te = 256, halo, align) for equal agglomerates: te - 2 halo rounded down to whole ones"""
    return ((TILE - 2 * halo) // align) * align


def _tile_ns(rho=4, npre=3, npost=3):
    """n at the ends of the two launches' owned ranges -> sorted list of (n, ratios); the ratios are (4, 2, 2) where 16
    divides n and (4,) -- two levels -- otherwise"""
    owned = {"descent": _owned(npre + 1, rho), "replay": _owned(npre + npost, 1)}
    ns = set()
    for o in owned.values():
        for k in (1, 2, 3):
            m = k * o
            m4 = -(-m // rho) * rho
            ns.update((m4, m4 + rho))                  # the multiple itself / a last tile owning one agglomerate
            ns.update(((m // 16) * 16, (m // 16 + 1) * 16))   # either side, with all three ratios
    return owned, [(n, RATIOS if n % 16 == 0 else (rho,)) for n in sorted(ns)]


OWNED, TILE_NS = _tile_ns()


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def arms(mg):
    """the three contexts: replay (the default, set explicitly) / the storing cycle / the plain kernels"""
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    for name, d, r in (("replay", 1, 1), ("store", 1, 0), ("plain", 0, 1)):
        ctx = mg.Context(0)
        ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, d)
        ctx.set_option(_lib.OPT_REPLAY_PRESMOOTH, r)
        out[name] = ctx
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _build(ctx, U, weights):
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    H = build_device_hierarchy(U, ctx)
    if weights is not None:
        H.set_sweep_weights(0, weights[0], weights[1])
    return H


def _run(ctx, U, b, x0, npre, npost, weights):
    """vcycle_dev x NCYC from x0 (None: no first iterate in the first cycle), ping-ponging x -> (x, replayed cycles);
    the first cycle's x0 must come back unchanged"""
    H = _build(ctx, U, weights)
    N = len(b)
    bd = ctx.to_device(b)
    before = ctx.replay_launches()
    xa, xb = ctx.alloc(N), ctx.alloc(N)
    first = None if x0 is None else ctx.to_device(x0)
    src = first
    for _ in range(NCYC):
        H.vcycle_dev(src, bd, xb, npre, npost)
        xa, xb = xb, xa
        src = xa
    x = xa.download()
    if first is not None:
        assert _same(first.download(), x0), "the cycle wrote to its first iterate"
    assert _same(bd.download(), b)
    count = ctx.replay_launches() - before
    H.free()
    return x, count


def _three(arms, U, b=None, x0=None, npre=3, npost=3, weights=None, replays=NCYC):
    b = U.rhs() if b is None else b
    xr, kr = _run(arms["replay"], U, b, x0, npre, npost, weights)
    xs, ks = _run(arms["store"], U, b, x0, npre, npost, weights)
    xp, kp = _run(arms["plain"], U, b, x0, npre, npost, weights)
    assert kr == replays, f"replayed cycles: {kr}, expected {replays}"
    assert ks == 0 and kp == 0, (ks, kp)
    assert np.all(np.isfinite(xp)) and np.any(xp != 0.0)
    for what, got, ref in (("replay / plain", xr, xp), ("store / plain", xs, xp)):
        assert _same(got, ref), (what, float(np.max(np.abs(got - ref))))
    return xr


def _hier(n, p=3, ratios=RATIOS, bc=None):
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    return UniformDgAggHierarchy(n, p=p, pAgg=1, ratios=ratios, bc=bc)


def test_planner_owned_ranges():
    """the owned ranges the shapes below are derived from"""
    print(f"owned per 256-element tile: {OWNED}; n: {[n for n, _ in TILE_NS]}")
    assert OWNED == {"descent": 248, "replay": 244}
    assert _owned(8, 1) == 240   # V(4, 4): all eight weights
    assert {240, 244, 248, 256, 488, 492, 496, 732, 736, 744} <= {n for n, _ in TILE_NS}


@pytest.mark.parametrize("n,ratios", TILE_NS)
def test_tile_edges_bitwise(mg, arms, n, ratios):
    """one tile exactly, a last tile owning one agglomerate, a last tile whose right halo lies wholly outside the level,
    n on both sides of the multiples of 244 / 248"""
    _three(arms, _hier(n, ratios=ratios))


@pytest.mark.parametrize("npre,npost", [(1, 1), (2, 3), (3, 1), (4, 4)])
def test_sweep_counts_bitwise(mg, arms, npre, npost):
    """other halos; (4, 4) fills all eight weights (halo 8)"""
    _three(arms, _hier(512), npre=npre, npost=npost)
    _three(arms, _hier(496), npre=npre, npost=npost,
           x0=np.random.default_rng(npre * 8 + npost).standard_normal(4 * 496))


@pytest.mark.parametrize("npre,npost", [(5, 4), (3, 0), (0, 3)])
def test_fallback_sweep_counts_bitwise(mg, arms, npre, npost):
    """more sweeps than weights of one launch, or none on one side: the storing cycle, counter 0"""
    _three(arms, _hier(512), npre=npre, npost=npost, replays=0)


def test_weight_order_bitwise(mg, arms):
    """six distinct weights, the pre-schedule different from the post-schedule: w_pre ++ w_post in the replaying launch"""
    w = (np.array([0.9, 0.5, 0.7]), np.array([0.3, 0.8, 0.6]))
    g = np.random.default_rng(3).standard_normal(4 * 512)
    _three(arms, _hier(512), weights=w)
    _three(arms, _hier(512), x0=g, weights=w)
    _three(arms, _hier(492, ratios=(4,)), x0=g[:4 * 492], npre=2, npost=3, weights=(w[0][:2], w[1]))


def test_first_iterate_bitwise(mg, arms):
    """no first iterate, explicit zeros (the same cycle) and a random one"""
    U = _hier(496)
    N = len(U.rhs())
    xn = _three(arms, U, x0=None)
    xz = _three(arms, U, x0=np.zeros(N))
    assert _same(xn, xz)
    _three(arms, U, x0=np.random.default_rng(11).standard_normal(N))


def test_exact_data_bitwise(mg, arms):
    """right-hand side and first iterate of exact small integers: a wrong element or row is a difference of order one"""
    U = _hier(496)
    N = len(U.rhs())
    rng = np.random.default_rng(5)
    b = rng.integers(-8, 9, N).astype(np.float64)
    g = rng.integers(-4, 5, N).astype(np.float64)
    _three(arms, U, b=b, x0=g)
    _three(arms, U, b=b)


@pytest.mark.parametrize("n", [240, 256])
def test_boundary_arrangements_bitwise(mg, arms, n):
    """Dirichlet left / Neumann right: the first and last elements' records change places"""
    _three(arms, _hier(n, bc=DIR_NEU))
    _three(arms, _hier(n, bc=DIR_NEU), x0=np.random.default_rng(n).standard_normal(4 * n))


@pytest.mark.parametrize("ratios,n", [((2, 2, 2, 2), 480), ((2, 2, 2, 2), 512), ((8, 2, 2), 480), ((8, 2, 2), 512)])
def test_other_fine_ratios_bitwise(mg, arms, ratios, n):
    """agglomerates of 2 and 8 elements: the prolongation's coarse index against a 4-element habit"""
    _three(arms, _hier(n, ratios=ratios), x0=np.random.default_rng(n).standard_normal(4 * n))


def test_overlapping_ranges_fall_back(mg, arms):
    """x_out partially overlapping x0 (offset by N / 2 inside one allocation of 2 N): the storing cycle, counter 0, the
    result of the call with disjoint vectors -- the replaying ascent would read x0's halos while x_out is stored"""
    U = _hier(496)
    b = U.rhs()
    N = len(b)
    g = np.random.default_rng(17).standard_normal(N)
    ctx = arms["replay"]
    H = _build(ctx, U, None)
    bd = ctx.to_device(b)
    ref = ctx.alloc(N)
    k0 = ctx.replay_launches()
    H.vcycle_dev(ctx.to_device(g), bd, ref)
    assert ctx.replay_launches() - k0 == 1
    for off in (N // 2, -(N // 2)):   # x_out behind x0, and in front of it
        big = ctx.to_device(np.concatenate([np.zeros(N // 2), g, np.zeros(N // 2)]))
        base = big.ptr.value
        x0p = base + (N // 2) * 8
        k0 = ctx.replay_launches()
        H.vcycle_dev(x0p, bd, x0p + off * 8)
        assert ctx.replay_launches() - k0 == 0
        lo = N // 2 + off
        assert _same(big.download()[lo:lo + N], ref.download()), off
    # adjacent ranges do not overlap: the cycle replays
    big = ctx.to_device(np.concatenate([g, np.zeros(N)]))
    k0 = ctx.replay_launches()
    H.vcycle_dev(big.ptr.value, bd, big.ptr.value + N * 8)
    assert ctx.replay_launches() - k0 == 1
    assert _same(big.download()[N:], ref.download())
    H.free()


def test_no_stale_state_bitwise(mg, arms):
    """a replayed cycle leaves nothing defined in the fine level's stored iterate: the loop over cycles and the next
    cycles on the same hierarchy must not see it"""
    U = _hier(736)
    b = U.rhs()
    N = len(b)
    g = np.random.default_rng(23).standard_normal(N)
    out = {}
    for name in ("replay", "store"):
        ctx = arms[name]
        H = _build(ctx, U, None)
        bd = ctx.to_device(b)
        xa, xb, xc = ctx.to_device(g), ctx.alloc(N), ctx.alloc(N)
        k0 = ctx.replay_launches()
        H.vcycle_dev(xa, bd, xb)            # replays
        H.vcycles_dev(xb, bd, xc, 2)        # the loop: the launch between its two cycles reads the stored iterate
        H.vcycle_dev(xc, bd, xa)            # replays again
        H.vcycles_dev(xa, bd, xb, 2)
        H.vcycle_dev(None, bd, xc)          # no first iterate: replays, reads no iterate at all
        out[name] = (xa.download(), xb.download(), xc.download(), ctx.replay_launches() - k0)
        H.free()
    assert out["replay"][3] == 3 and out["store"][3] == 0
    for a, s in zip(out["replay"][:3], out["store"][:3]):
        assert _same(a, s)


def test_half_cycles_keep_the_stored_iterate(mg, arms):
    """the one reader of the stored iterate across calls is an ascent on its own after a whole cycle: refused right
    after a replayed cycle (nothing was stored), and once a half-cycle entry point has been called on a hierarchy its
    cycles store -- counter 0 -- so that descent + ascent, and a whole cycle + ascent, give the storing context's bits"""
    U = _hier(736)
    b = U.rhs()
    N = len(b)
    g = np.random.default_rng(29).standard_normal(N)
    out = {}
    for name in ("replay", "store"):
        ctx = arms[name]
        H = _build(ctx, U, None)
        bd, gd = ctx.to_device(b), ctx.to_device(g)
        xa, xb, xc = ctx.alloc(N), ctx.alloc(N), ctx.alloc(N)
        k0 = ctx.replay_launches()
        H.vcycle_dev(gd, bd, xa)
        first = ctx.replay_launches() - k0
        if name == "replay":
            assert first == 1
            with pytest.raises(mg.ArgumentError, match="replayed its pre-smoothing"):
                H.vcycle_up_dev(bd, xb)
        else:
            assert first == 0
        k0 = ctx.replay_launches()
        H.vcycle_down_dev(gd, bd)
        H.vcycle_dev(gd, bd, xa)     # (the coarsest solve of a whole cycle, then the ascent alone: the same x)
        H.vcycle_up_dev(bd, xb)
        H.vcycle_dev(None, bd, xc)
        assert ctx.replay_launches() - k0 == 0
        out[name] = (xa.download(), xb.download(), xc.download())
        assert _same(out[name][0], out[name][1])
        H.free()
    for a, s in zip(out["replay"], out["store"]):
        assert _same(a, s)


def test_launch_bytes_of_the_replay_forms(mg, arms):
    """the descent without its 32 B per element store; the ascent reads the first iterate where the storing one reads the
    stored iterate, or none.  'down' / 'up' keep describing the storing launches"""
    ne = 1024
    H = _build(arms["replay"], _hier(ne), None)
    rd, wd = H.launch_bytes(0, "down")
    ru, wu = H.launch_bytes(0, "up")
    assert H.launch_bytes(0, "replay_down") == (rd, wd - 32 * ne)
    assert H.launch_bytes(0, "replay_up") == (ru, wu)
    assert H.launch_bytes(0, "replay_down", has_x0=False) == (rd - 32 * ne, wd - 32 * ne)
    assert H.launch_bytes(0, "replay_up", has_x0=False) == (ru - 32 * ne, wu)
    H.free()
