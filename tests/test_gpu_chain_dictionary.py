"""Operator dictionary of the CG chain levels (AGGMG_OPT_OPERATOR_DICTIONARY; csrc/cgt_kernels.hpp
cgt_fused_kernel<..., DICT = true>, set-up csrc/setup.hip setup_cgt_dictionary): on a uniform mesh the per-block records
of a chain level -- the block's rows of dblk / subrow / supcol and of its transfer -- repeat, the level keeps one copy of
every distinct record and the point-Jacobi launches of a cycle index operator and transfer by the block's class.  The
loads return the operator's own bits from another address, so every result must equal the run with the option off BIT
FOR BIT (compared as 64-bit patterns: stricter than ==, and indifferent to what the values are).  The tests switch the
option on and off explicitly; every case runs vcycle_dev x 3 and vcycles_dev(3) (the launch between two cycles)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _ctx(mg, on):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_OPERATOR_DICTIONARY, 1 if on else 0)
    return ctx


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _run(mg, build, on, x0=None, ncyc=3, nPre=3, nPost=3, alpha=2.0 / 3.0):
    """vcycle_dev x ncyc and vcycles_dev(ncyc) from x0 (None: the zero guess) -> (x, x of the loop, dictionary levels)"""
    ctx = _ctx(mg, on)
    H, b = build(ctx)
    N = len(b)
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(np.zeros(N) if x0 is None else x0), ctx.alloc(N)
    for _ in range(ncyc):
        H.vcycle_dev(xa, bd, xb, nPre, nPost, alpha)
        xa, xb = xb, xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N) if x0 is None else x0), bd, xb, ncyc, nPre, nPost, alpha)
    xl = xb.download()
    levels = H.dictionary_levels()
    H.free()
    return x, xl, levels


def _on_off(mg, build, **kw):
    x1, xl1, lv1 = _run(mg, build, True, **kw)
    x0_, xl0, lv0 = _run(mg, build, False, **kw)
    assert lv0 == {}, lv0
    assert _same(x1, x0_), float(np.max(np.abs(x1 - x0_)))
    assert _same(xl1, xl0) and _same(xl1, x1)
    return lv1


def _uniform(U, smoother="jac"):
    from agglomerationmultigrid1d_amd.uniform import build_device_cg_hierarchy
    return lambda ctx: (build_device_cg_hierarchy(U, ctx, smoother=smoother), U.rhs())


def _detected(U):
    """operators only, no element lists: the library recognises the chains itself (what tools/exp_cg_chain.py --detect
    builds; build_device_cg_hierarchy(chain=True) always hands the lists over)"""
    def build(ctx):
        import agglomerationmultigrid1d_amd as mg
        from agglomerationmultigrid1d_amd import _lib
        ops = [mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx) for A in U.A]
        sms = [mg.JacobiSmoother(ops[k], ctx, None, detect=True) for k in range(U.nlevels - 1)]
        Ls = [mg.DeviceOperator(L, _lib.OP_TRANSFER, ctx) for L in U.L]
        H = mg.MeshHierarchy(None, ops, sms, Ls, ctx=ctx)
        assert H.level_kinds() == ['fused_chain'] * (U.nlevels - 1) + ['coarsest'], H.level_kinds()
        return H, U.rhs()
    return build


def _block_order(n, p):
    """reference numbering (vertices 0..n, then p - 1 interior nodes per element) -> index in block order (block e =
    vertex e and the interior nodes of element e; the trailing block holds vertex n alone)"""
    inv = np.empty(n * p + 1, dtype=np.int64)
    inv[:n + 1] = np.arange(n + 1) * p
    if p > 1:
        e, j = np.divmod(np.arange(n * (p - 1)), p - 1)
        inv[n + 1:] = e * p + 1 + j
    return inv


def _cpu_classes(U, k):
    return _input_classes(U.n, U.ps, U.A, U.L, k)


def _input_classes(n, ps, As, Ls, k):
    """distinct per-block INPUT records of CG level k (n elements, degrees ps, operators and transfers in the reference
    numbering): the three block rows of A and the block's rows of L, as 64-bit patterns, over all n + 1 blocks -- the
    trailing block that holds the last vertex alone is one of them, so a mesh with a first, an interior and a last
    element counts 4.  The device record stores every one of these entries, so the device has at least as many classes."""
    p = ps[k]
    inv = _block_order(n, p)
    A = As[k].tocoo()
    rb, cb = inv[A.row], inv[A.col]
    e = rb // p
    rec = np.zeros((n + 1, p, 3 * p))
    rec[e, rb - e * p, cb - e * p + p] = A.data
    L = Ls[k].tocoo()
    rb = inv[L.row]
    e = rb // p
    if k + 1 < len(ps):                 # chain transfer: coarse block e and the first DoF of coarse block e + 1
        mc = ps[k + 1]
        slot = _block_order(n, mc)[L.col] - e * mc
        lrec = np.zeros((n + 1, p, mc + 1))
    else:                                 # into the DG p = 0 level: element e and, from the vertex, element e - 1
        slot = L.col - e + 1
        lrec = np.zeros((n + 1, p, 2))
    assert slot.min() >= 0 and slot.max() < lrec.shape[2]
    lrec[e, rb - e * p, slot] = L.data
    both = np.concatenate([rec.reshape(n + 1, -1), lrec.reshape(n + 1, -1)], axis=1)
    return len(np.unique(np.ascontiguousarray(both).view(np.uint64), axis=0))


def _check_config5(U, lv, n):
    cpu = {k: _cpu_classes(U, k) for k in range(3)}
    print(f"n={n}: device classes per level {lv}, CPU input classes {cpu}")
    for k in range(3):
        assert k in lv, (k, lv)
        assert 1 <= lv[k] <= min(n + 1, 1024), lv
        assert cpu[k] <= lv[k], (cpu, lv)
        if n == 4096:
            assert lv[k] <= 16, lv


@pytest.mark.parametrize("n", [16, 48, 256, 384, 4096])
def test_config5_cycles_bitwise(mg, n):
    """BASELINE config 5's hierarchy (CG p = 4, 2, 1, then DG p = 0): 17 blocks (less than one tile, both ends in it),
    non-dyadic counts with 17 / 26 input classes (48, 384; the trailing block counted), 257 blocks (several tiles of 64 blocks on the p = 4 level, one
    cut by the end), the dyadic case at 4096.  All three chain levels must have a dictionary."""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(n)
    _check_config5(U, _on_off(mg, _uniform(U)), n)


def test_nonzero_guess_and_halves_bitwise(mg):
    """a non-zero first guess, the zero guess given as x0 = None, and the two halves of the cycle called on their own
    (descent: sweeps, residual, restriction; ascent: prolongation, sweeps), the coarsest right-hand side compared"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, build_device_cg_hierarchy
    U = UniformCgDgHierarchy(4096)
    b = U.rhs()
    g = np.random.default_rng(7).standard_normal(len(b))
    lv = _on_off(mg, _uniform(U), x0=g)
    assert all(k in lv for k in range(3)), lv
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_cg_hierarchy(U, ctx)
        bd, xd = ctx.to_device(b), ctx.alloc(len(b))
        res = []
        for guess in (g, np.zeros(len(b))):
            H.vcycle_down_dev(ctx.to_device(guess), bd)
            rhs_ptr, sol_ptr, nc = H.coarse_buffers()
            rc = np.empty(nc)
            ctx.synchronize()
            ctx.check(ctx.lib.aggmg_memcpy_d2h(ctx.handle, rc.ctypes.data, rhs_ptr, nc * 8))
            res.append(rc)
        H.vcycle_dev(None, bd, xd)               # x0 = None: the zero guess, the fine level reads no iterate
        res.append(xd.download())
        H.vcycle_dev(ctx.to_device(g), bd, xd)   # (leaves a coarsest solution for the ascent alone)
        H.vcycle_up_dev(bd, xd)
        res.append(xd.download())
        out.append(res)
        H.free()
    for r1, r0 in zip(*out):
        assert _same(r1, r0)


@pytest.mark.parametrize("nPre,nPost,alpha", [(0, 0, 2.0 / 3.0), (0, 3, 2.0 / 3.0), (3, 0, 2.0 / 3.0), (1, 2, 0.5), (11, 9, 2.0 / 3.0)],
                         ids=["V00", "V03", "V30", "V12-alpha0.5", "V11-9-chunked"])
def test_sweep_counts_bitwise(mg, nPre, nPost, alpha):
    """no sweeps on one side or on both (the launch is the residual + restriction, or the prolongation, alone), and more
    sweeps than one launch takes: the sweeps are chunked and the intermediate launches index by class too"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(384)
    lv = _on_off(mg, _uniform(U), nPre=nPre, nPost=nPost, alpha=alpha)
    assert all(k in lv for k in range(3)), lv


def _reference(Ho, b):
    def build(ctx):
        import agglomerationmultigrid1d_amd as mg
        return mg.MeshHierarchy.from_reference(Ho, ctx=ctx), b
    return build


def test_agglomerating_transfer_and_other_block_sizes_bitwise(oracle, mg):
    """the oracle's builders (at most 1024 blocks per level: a dictionary always exists where the level is eligible).
    CG 8, 4, 2, 1 then agglomerated levels: blocks of 8 rows keep the full arrays, the p = 4, 2, 1 levels take the form,
    the last of them restricting into 4:1 agglomerates.  CG 6, 3: no chain level takes it."""
    o = oracle
    Ho, b = o.build_cg_hierarchy(64, ps=(8, 4, 2, 1), nAgg=5)
    lv = _on_off(mg, _reference(Ho, b))
    print(f"ps=(8,4,2,1) nAgg=5: classes per level {lv}")
    assert 0 not in lv, lv
    assert all(k in lv for k in (1, 2, 3)), lv
    Ho, b = o.build_cg_hierarchy(96, ps=(6, 3), nDG=2, pDG=1)
    lv = _on_off(mg, _reference(Ho, b))
    print(f"ps=(6,3) nDG=2 pDG=1: classes per level {lv}")
    assert 0 not in lv and 1 not in lv, lv


def test_many_classes_bitwise(mg):
    """a uniform mesh of an interval whose vertices round in many different ways (the mesh that overflows the DG
    dictionary): on the chain levels it gives on the order of a hundred classes -- the element matrices depend on the
    element's width alone -- and their number grows with the logarithm of n (CPU count of the fine level: 109 at
    n = 160000, 144 at 10^6, 150 at 3 10^6), so the levels take the form with class numbers far beyond a handful"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    n = 160000
    U = UniformCgDgHierarchy(n, xin=-1.0 / 3.0, xout=1.0e9 + 0.7)
    lv = _on_off(mg, _uniform(U))
    cpu = {k: _cpu_classes(U, k) for k in range(3)}
    print(f"n={n}: device classes per level {lv}, CPU input classes {cpu}")
    for k in range(3):
        assert k in lv and cpu[k] <= lv[k] <= 1024, (cpu, lv)


def test_too_many_classes_keeps_the_full_arrays(oracle, mg, monkeypatch):
    """more distinct records than the dictionary takes (counted on the CPU first), so the chain levels keep the plain
    path.  The rounding mesh of test_many_classes_bitwise cannot get there by a larger n (see its figures); here every
    interior vertex of the oracle's mesh is moved by a random fraction of the element width, 1200 elements: every block
    has a record of its own."""
    o = oracle
    n, ps = 1200, (4, 2, 1)
    uniform = o.create_uniform_mesh

    def jittered(n_, xin, xout):
        mesh = uniform(n_, xin, xout)
        d = np.random.default_rng(5).uniform(-0.3, 0.3, n_ + 1) * (xout - xin) / n_
        for v, dv in zip(mesh.mVertices[1:-1], d[1:-1]):
            v.mX += dv
        return mesh
    monkeypatch.setattr(o, "create_uniform_mesh", jittered)
    Ho, b = o.build_cg_hierarchy(n, ps=ps, nDG=1, pDG=0)
    ncpu = _input_classes(n, ps, Ho.mStiffness, Ho.mInterpolation, 0)
    print(f"CPU input classes of the fine level {ncpu}")
    assert ncpu > 1024
    lv = _on_off(mg, _reference(Ho, b))
    assert all(k not in lv for k in range(3)), lv


def test_multigrid_with_checkpoints_bitwise(mg):
    """the device-resident loop with the checkpoint on: its fine launches keep the full arrays; histories compared too"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy, build_device_cg_hierarchy
    U = UniformCgDgHierarchy(4096)
    b = U.rhs()
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        ctx.set_option(_lib.OPT_MG_CHECKPOINT, 1)
        H = build_device_cg_hierarchy(U, ctx)
        assert (0 in H.dictionary_levels()) == on
        res = []
        for every in (1, 3):
            x, it, r = mg.multigrid_dev(H, ctx.to_device(np.zeros(len(b))), ctx.to_device(b), 9, 1e-30, check_every=every)
            res.append((x.download(), it, list(r)))
        out.append(res)
        H.free()
    for (x1, it1, r1), (x0, it0, r0) in zip(*out):
        assert it1 == it0 and r1 == r0
        assert _same(x1, x0)


@pytest.mark.parametrize("smoother", ["addSchwarz", "hybridSchwarz", "blockGS"])
def test_element_smoothers_keep_the_full_arrays_bitwise(mg, smoother):
    """element Schwarz and red-black element Gauss-Seidel levels: their records (the element inverses) are not in the
    dictionary, so no chain level has one and the launches read the full arrays"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(384)
    alpha = {"addSchwarz": 0.5, "hybridSchwarz": 1.0, "blockGS": 1.0}[smoother]
    lv = _on_off(mg, _uniform(U, smoother=smoother), alpha=alpha)
    assert all(k not in lv for k in range(3)), lv


def test_operator_level_entries_bitwise(mg):
    """sweeps and the residual on a chain operator without a hierarchy: the full arrays, the same bits on and off"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    U = UniformCgDgHierarchy(384)
    N = U.A[0].shape[0]
    rng = np.random.default_rng(11)
    u, b = rng.standard_normal(N), rng.standard_normal(N)
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        op = mg.DeviceOperator(U.A[0], _lib.OP_STIFFNESS, ctx)
        S = mg.JacobiSmoother(op, ctx, U.element_nodes(0))
        assert S.structured
        out.append([mg.smooth(op, S, u, b, 2.0 / 3.0, ns) for ns in (3, 19)] + [mg.residual(op, u, b)])
    for r1, r0 in zip(*out):
        assert _same(r1, r0)


def test_chain_detected_from_the_operators_alone_bitwise(mg):
    """no element lists: the chains are recognised from the operators' patterns, and the levels take the form as well"""
    from agglomerationmultigrid1d_amd.uniform import UniformCgDgHierarchy
    n = 256
    U = UniformCgDgHierarchy(n)
    _check_config5(U, _on_off(mg, _detected(U)), n)
