"""A V-cycle through generic levels IS its parts: on a hierarchy whose non-coarsest levels all run the generic kernels, one
aggmg_vcycle_dev equals, BIT FOR BIT, the cycle of src/solvers.jl:28-47 composed from the stand-alone entry points --
aggmg_smooth_dev (distinct input and output), aggmg_residual_dev, aggmg_restrict_dev, aggmg_prolong_add_dev -- and a
one-level hierarchy's solve of the coarsest operator.  The cycle driver builds its generic half-cycles on the sweep runner
aggmg_smooth_dev uses; this pins that the two cannot drift apart (vectors, scratch slots, sweep order, damping).

Point Jacobi on CG operators in the reference's vertices-first numbering (not banded: CSR sweeps, one per launch) and
additive / hybrid element Schwarz on lists in a scrambled order (off the chain kernel: block sweep + combine, the same
two launches whatever aliases).  300 fine elements: more than 256 rows and more than 256 / 5 blocks on every smoothed
level, so every kernel runs several workgroups.  Banded point Jacobi as well (DG p = 3 and its agglomerated levels under
dg_smoother(:jac); 304 elements, the ratios 4, 2, 2 want a multiple of 16): on the way down its residual comes out of the
sweeps' launch -- another kernel than aggmg_residual_dev -- with the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ELEMS = 300
SWEEPS = [(3, 3), (0, 2), (2, 0)]
ALPHA = 0.5   # (tests/cg_smoother_test.jl: additive Schwarz wants <= 1/2; the others take it too)


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def build(mg, ctx, smoother):
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, UniformDgAggHierarchy, build_device_cg_hierarchy
    if smoother == "bandJac":
        U = UniformDgAggHierarchy(N_ELEMS + 4, p=3, pAgg=1, ratios=(4, 2, 2))
        ops = [mg.DeviceOperator(U.stiffness_csc(k), _lib.OP_STIFFNESS, ctx) for k in range(U.nlevels)]
        sms = [mg.JacobiSmoother(op, ctx, detect=False) for op in ops[:-1]]
        Ls = [mg.DeviceOperator(U.interpolation_csc(k), _lib.OP_TRANSFER, ctx) for k in range(U.nlevels - 1)]
        return mg.MeshHierarchy(None, ops, sms, Ls, ctx=ctx), U.rhs()
    U = UniformCgDgHierarchy(N_ELEMS, ps=(4, 2, 1))
    if smoother == "jac":
        return build_device_cg_hierarchy(U, ctx, chain=False), U.rhs()
    cls = {"addSchwarz": mg.AdditiveSchwarzSmoother, "hybridSchwarz": mg.HybridSchwarzSmoother}[smoother]
    ops = [mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx) for A in U.A]
    sms = []
    for k in range(U.nlevels - 1):
        el = U.element_nodes(k)
        sms.append(cls(ops[k], np.ascontiguousarray(el[:, np.random.default_rng(k).permutation(el.shape[1])]), ctx))
    Ls = [mg.DeviceOperator(L, _lib.OP_TRANSFER, ctx) for L in U.L]
    return mg.MeshHierarchy(None, ops, sms, Ls, ctx=ctx), U.rhs()


def composed_cycle(mg, H, x0, b, nPre, nPost, alpha):
    """src/solvers.jl:28-47 from the stand-alone device entry points -> DeviceVector"""
    ctx, n = H.ctx, H.nlevels
    lib, c = ctx.lib, ctx.handle
    ops, sms, Ls = H._ops, H.mSmoothers, H._Ls
    u, rhs = [None] * n, [b] + [None] * (n - 1)
    for k in range(n - 1):
        N = ops[k].shape[0]
        u[k], r, rhs[k + 1] = ctx.alloc(N), ctx.alloc(N), ctx.alloc(ops[k + 1].shape[0])
        u_in = x0.ptr if k == 0 else None    # u[k] = zeros below the finest level (:29-31)
        ctx.check(lib.aggmg_smooth_dev(c, ops[k].handle, sms[k].handle, u_in, rhs[k].ptr, alpha, nPre, u[k].ptr))
        ctx.check(lib.aggmg_residual_dev(c, ops[k].handle, u[k].ptr, rhs[k].ptr, r.ptr))
        ctx.check(lib.aggmg_restrict_dev(c, Ls[k].handle, r.ptr, rhs[k + 1].ptr))
    Hc = mg.MeshHierarchy(None, [ops[-1]], [], [], ctx=ctx)    # the coarsest solve (:39)
    u[n - 1] = ctx.alloc(ops[-1].shape[0])
    Hc.vcycle_dev(None, rhs[n - 1], u[n - 1], 0, 0, alpha)
    for k in range(n - 2, -1, -1):
        ctx.check(lib.aggmg_prolong_add_dev(c, Ls[k].handle, u[k + 1].ptr, u[k].ptr))
        out = ctx.alloc(ops[k].shape[0])
        ctx.check(lib.aggmg_smooth_dev(c, ops[k].handle, sms[k].handle, u[k].ptr, rhs[k].ptr, alpha, nPost, out.ptr))
        u[k] = out
    ctx.synchronize()
    Hc.free()
    return u[0]


def cycle_and_composition(mg, H, b_host, nPre, nPost):
    ctx = H.ctx
    N = len(b_host)
    b = ctx.to_device(b_host)
    x0 = ctx.to_device(np.cos(0.37 * np.arange(N)))
    out = ctx.alloc(N)
    H.vcycle_dev(x0, b, out, nPre, nPost, ALPHA)
    return out.download(), composed_cycle(mg, H, x0, b, nPre, nPost, ALPHA).download()


@pytest.fixture(scope="module", params=["jac", "addSchwarz", "hybridSchwarz", "bandJac"])
def hierarchy(mg, request):
    H, b = build(mg, mg.Context(0), request.param)
    assert H.level_kinds() == ["generic"] * 3 + ["coarsest"], H.level_kinds()
    yield H, b
    H.free()


@pytest.mark.parametrize("nPre,nPost", SWEEPS)
def test_vcycle_through_generic_levels_is_the_composition_of_its_parts(mg, hierarchy, nPre, nPost):
    H, b = hierarchy
    got, want = cycle_and_composition(mg, H, b, nPre, nPost)
    assert np.all(np.isfinite(got)) and np.linalg.norm(got) > 0.0
    diff = float(np.max(np.abs(got - want)))
    print(f"nPre={nPre} nPost={nPost}: max |cycle - composition| = {diff:.3e}")
    assert np.array_equal(got, want), diff
