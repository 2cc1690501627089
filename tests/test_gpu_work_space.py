"""The context's shared work space (csrc/workspace.hpp: the leased vectors ctx->solv / ctx->scratch, the named scalars):
every entry point that uses it, one after the other on ONE context, gives the bits it gives on a context of its own --
in either order, after the buffers have grown for a larger problem, and after they have been left larger than the
problem needs.

The sequence (ITEMS): pcg; pcg on K = 3 columns; multigrid with a check after every cycle and the error history (the
checks formed inside the fine-level launch), the same with AGGMG_OPT_MG_CHECKPOINT = 0 (a residual launch per check); the
smoother solve on the block-tridiagonal operator and on the CG chain operator; fgmres(5); estimate_lambda_max;
aggmg_smooth_dev in place with more sweeps than one fused launch takes (a launch's weight array holds
MAX_SWEEP_WEIGHTS of them); one sweep of an overlapping additive Schwarz smoother through the generic kernels.

Shapes: the DG hierarchy p = 3 -> 4:1 -> 2:1 -> 2:1 at 256 and at 1024 fine elements, the CG chain 4 -> 2 -> 1 at 96."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, LARGE, CG_ELEMS = 256, 1024, 96
ALPHA = 2.0 / 3.0


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


_MESH = {}


def mesh(key):
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, UniformDgAggHierarchy
    if key not in _MESH:
        _MESH[key] = UniformCgDgHierarchy(CG_ELEMS, ps=(4, 2, 1)) if key == "cg" else \
            UniformDgAggHierarchy(key, p=3, pAgg=1, ratios=(4, 2, 2))
    return _MESH[key]


class World:
    """the device objects of one problem size on one context, built when first asked for"""

    def __init__(self, mg, ctx, n):
        self.mg, self.ctx, self.n = mg, ctx, n
        self._dg = self._cg = self._schwarz = None
        self.b = mesh(n).rhs()
        self.N = len(self.b)
        rng = np.random.default_rng(n)
        self.B = np.asfortranarray(rng.standard_normal((self.N, 3)))
        self.u0 = rng.standard_normal(self.N)

    @property
    def dg(self):
        from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
        if self._dg is None:
            self._dg = build_device_hierarchy(mesh(self.n), self.ctx)
            assert self._dg.level_kinds()[0] == "fused_btd", self._dg.level_kinds()
        return self._dg

    @property
    def cg(self):
        from agglomerationmultigrid1d_amd.uniform import build_device_cg_hierarchy
        if self._cg is None:
            self._cg = build_device_cg_hierarchy(mesh("cg"), self.ctx)
            assert self._cg.level_kinds()[0] == "fused_chain", self._cg.level_kinds()
        return self._cg

    @property
    def schwarz(self):
        """pairs of neighbouring elements of the fine DG operator: every inner element lies in two blocks"""
        if self._schwarz is None:
            inds = 4 * np.arange(self.n - 1)[None, :] + np.arange(8)[:, None] + 1     # (m, nb), 1-based
            self._schwarz = self.mg.AdditiveSchwarzSmoother(self.dg._ops[0], inds, self.ctx)
        return self._schwarz

    def free(self):
        if self._schwarz is not None:
            self._schwarz.free()
        for H in (self._dg, self._cg):
            if H is None:
                continue
            for owner in [H] + list(H.mSmoothers):       # (exact=True keeps a direct solver with its owner)
                ds = owner.__dict__.pop("_direct_solver", None)
                if ds is not None and ds.H is not None:
                    ds.H.free()
            H.free()
            for obj in list(H.mSmoothers) + H._ops + H._Ls:
                obj.free()


def _multigrid(w, checkpoint):
    from agglomerationmultigrid1d_amd import _lib
    was = w.ctx.option(_lib.OPT_MG_CHECKPOINT, 1)
    w.ctx.set_option(_lib.OPT_MG_CHECKPOINT, checkpoint)
    try:
        x, it, res, err = w.mg.multigrid(w.dg, np.zeros(w.N), w.b, 5, 1e-13, exact=True, check_every=1)
    finally:
        w.ctx.set_option(_lib.OPT_MG_CHECKPOINT, was)
    assert it == len(res) == len(err) and it >= 2
    return x, it, res, err


def _smooth_in_place(w):
    from agglomerationmultigrid1d_amd import _lib
    c = w.ctx
    H = w.dg
    u, bd = c.to_device(w.u0), c.to_device(w.b)
    nsweeps = _lib.MAX_SWEEP_WEIGHTS + 3
    c.check(c.lib.aggmg_smooth_dev(c.handle, H._ops[0].handle, H.mSmoothers[0].handle, u.ptr, bd.ptr, ALPHA, nsweeps, u.ptr))
    c.synchronize()
    return (u.download(),)


ITEMS = [
    ("pcg", lambda w: w.mg.pcg(w.dg, w.b, maxiter=6, tol=1e-10)),
    ("pcg_K3", lambda w: w.mg.pcg(w.dg, w.B, maxiter=6, tol=1e-10)),
    ("multigrid_checkpointed", lambda w: _multigrid(w, 1)),
    ("multigrid_residual_launches", lambda w: _multigrid(w, 0)),
    ("smoother_solve_btd", lambda w: w.mg.iterative_smoother_solve(w.dg._ops[0], w.dg.mSmoothers[0], np.zeros(w.N), w.b, maxiter=12,
                                                                  tol=1e-30, alpha=ALPHA, exact=True, check_every=1)),
    ("smoother_solve_chain", lambda w: w.mg.iterative_smoother_solve(w.cg._ops[0], w.cg.mSmoothers[0], np.zeros(len(mesh("cg").rhs())),
                                                                    mesh("cg").rhs(), maxiter=12, tol=1e-30, alpha=ALPHA,
                                                                    exact=True, check_every=3)),
    ("fgmres_5", lambda w: w.mg.fgmres(w.dg, w.b, restart=5, maxiter=12, tol=1e-10)),
    ("lambda_max", lambda w: (w.dg.estimate_lambda_max(0, iters=10),)),
    ("smooth_in_place_chunked", _smooth_in_place),
    ("schwarz_sweep", lambda w: (w.mg.smooth(w.dg._ops[0], w.schwarz, w.u0, w.b, alpha=0.5, nsweeps=1),)),
]


def as_bytes(result):
    """a result tuple -> its bytes: arrays, counts and histories (lists, or one list per column)"""
    out = []
    for v in result:
        if isinstance(v, (list, tuple)) and v and isinstance(v[0], (list, tuple)):
            out.append(b"|".join(np.asarray(col, dtype=np.float64).tobytes() for col in v))
        else:
            out.append(np.ascontiguousarray(np.asarray(v, dtype=np.float64)).tobytes())
    return out


_ALONE = {}


def alone(mg, n, k):
    """item k at size n on a context of its own: computed once, shared by the cases"""
    if (n, k) not in _ALONE:
        ctx = mg.Context(0)
        w = World(mg, ctx, n)
        try:
            _ALONE[(n, k)] = as_bytes(ITEMS[k][1](w))
        finally:
            w.free()
            ctx.close()
    return _ALONE[(n, k)]


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_one_context_gives_the_bits_of_fresh_contexts(mg, order):
    from agglomerationmultigrid1d_amd.api import device_memory
    ks = list(range(len(ITEMS)))
    if order == "reverse":
        ks.reverse()
    ctx = mg.Context(0)
    worlds = {n: World(mg, ctx, n) for n in (SMALL, LARGE)}
    try:
        for n in (SMALL, LARGE, SMALL):     # the slots are taken, grow, and are then larger than asked for
            for k in ks:
                got = as_bytes(ITEMS[k][1](worlds[n]))
                want = alone(mg, n, k)
                assert len(got) == len(want), (ITEMS[k][0], n)
                for i, (g, x) in enumerate(zip(got, want)):
                    assert g == x, f"{ITEMS[k][0]} at {n} elements ({order}): output {i} differs from a fresh context's"
        print(f"device memory after the {order} sequence (allocations, bytes): {device_memory()}")
    finally:
        for w in worlds.values():
            w.free()
        ctx.close()
