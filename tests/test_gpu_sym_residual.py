"""Lossless symmetric form of the explicit residual's entries (AGGMG_OPT_SYMMETRIC_RESIDUAL, csrc/kernels.hpp
sym_residual_row): the fused descent reads the upper triangle of each diagonal block plus one word of int8 corrections
per row, and rebuilds every lower entry and every coupling entry from its mirror's bit pattern.  The entries are the
operator's own bits, so every result must equal the run with the option off BIT FOR BIT.  (The tests switch it on
and off explicitly.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


def _ctx(mg, on):
    from agglomerationmultigrid1d_amd import _lib
    ctx = mg.Context(0)
    ctx.set_option(_lib.OPT_SYMMETRIC_RESIDUAL, 1 if on else 0)
    return ctx


def _cycles(mg, U, on, ncyc, smoother="blockJac"):
    from agglomerationmultigrid1d_amd.uniform import build_device_hierarchy
    ctx = _ctx(mg, on)
    H = build_device_hierarchy(U, ctx, smoother=smoother)
    b = U.rhs()
    N = len(b)
    bd = ctx.to_device(b)
    xa, xb = ctx.to_device(np.zeros(N)), ctx.alloc(N)
    for _ in range(ncyc):
        H.vcycle_dev(xa, bd, xb)
        xa, xb = xb, xa
    x = xa.download()
    H.vcycles_dev(ctx.to_device(np.zeros(N)), bd, xb, ncyc)
    xl = xb.download()
    levels = H.sym_residual_levels()
    H.free()
    return x, xl, levels


@pytest.mark.parametrize("n,ncyc", [(2**16, 1), (2**16, 3), (2**20, 1), (2**20, 3)])
def test_config34_cycles_bitwise(mg, n, ncyc):
    """the benchmark's hierarchy (DG p = 3, then 4:1, 2:1, 2:1): the fine level takes the symmetric form"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=(4, 2, 2))
    x1, xl1, lv1 = _cycles(mg, U, True, ncyc)
    x0, xl0, lv0 = _cycles(mg, U, False, ncyc)
    assert lv1 == [0] and lv0 == [], (lv1, lv0)
    assert np.array_equal(x1, x0), float(np.max(np.abs(x1 - x0)))
    assert np.array_equal(xl1, xl0) and np.array_equal(xl1, x1)


@pytest.mark.parametrize("p", [1, 2, 3, 4])
def test_polynomial_degrees_bitwise(mg, p):
    """p = 3 (blocks of 4) takes the symmetric form; p = 1 (its pairs do not fit an int8) and p = 2 / 4 (block sizes
    of the lane-group path only) keep the full arrays -- the results are the same bits either way"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(2**14, p=p, pAgg=1, ratios=(4, 2, 2))
    x1, xl1, lv1 = _cycles(mg, U, True, 2)
    x0, xl0, lv0 = _cycles(mg, U, False, 2)
    print(f"p={p}: levels with the symmetric residual form {lv1}")
    assert lv0 == []
    assert lv1 == ([0] if p == 3 else []), lv1
    assert np.array_equal(x1, x0) and np.array_equal(xl1, xl0)


@pytest.mark.parametrize("n", [2**14, 2**16 + 16])
def test_block_gauss_seidel_bitwise(mg, n):
    """red-black block Gauss-Seidel levels: the form is built, the Gauss-Seidel variant of the fused kernel keeps reading
    the full arrays -- the same bits either way"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=(4, 2, 2))
    x1, xl1, lv1 = _cycles(mg, U, True, 2, smoother="blockGS")
    x0, xl0, lv0 = _cycles(mg, U, False, 2, smoother="blockGS")
    assert lv1 == [0] and lv0 == [], (lv1, lv0)
    assert np.array_equal(x1, x0), float(np.max(np.abs(x1 - x0)))
    assert np.array_equal(xl1, xl0)


@pytest.mark.parametrize("checkpoint", [1, 0])
def test_smoother_solve_bitwise(mg, checkpoint):
    """aggmg_smoother_solve_dev: several checkpoints inside each sweep launch (AGGMG_OPT_MG_CHECKPOINT = 1), or sweep
    launches and residual launches of their own (0: the residual launches read the symmetric form)"""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    U = UniformDgAggHierarchy(3000, p=3, pAgg=1, ratios=())
    b = U.rhs()
    N = len(b)
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        ctx.set_option(_lib.OPT_MG_CHECKPOINT, checkpoint)
        op = mg.DeviceOperator(U.stiffness_csc(0), _lib.OP_STIFFNESS, ctx)
        S = mg.BlockJacobi(op, U.descriptor(0).mBlockInds, ctx)
        for every in (1, 3):
            x, it, res, _ = mg.smoother_solve_dev(op, S, ctx.to_device(np.zeros(N)), ctx.to_device(b), 12, 1e-30,
                                                  2.0 / 3.0, check_every=every)
            out.append((on, every, x.download(), it, list(res)))
    half = len(out) // 2
    for (_, e1, x1, it1, r1), (_, e0, x0, it0, r0) in zip(out[:half], out[half:]):
        assert e1 == e0 and it1 == it0 == 12 and len(r1) == len(r0) > 0
        assert r1 == r0
        assert np.array_equal(x1, x0)


def test_ragged_hierarchy_bitwise(mg):
    """perturbed fine mesh (its entries' mirror differences are not those of the uniform mesh), agglomerates of
    different sizes below"""
    from agglomerationmultigrid1d_amd.uniform import build_device_ragged_hierarchy
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H, b, _ = build_device_ragged_hierarchy(2**16, ctx)
        N = len(b)
        bd = ctx.to_device(b)
        xb = ctx.alloc(N)
        H.vcycles_dev(ctx.to_device(np.zeros(N)), bd, xb, 3)
        out.append((xb.download(), H.sym_residual_levels()))
        H.free()
    (x1, lv1), (x0, lv0) = out
    assert lv1 == [0] and lv0 == []
    assert np.array_equal(x1, x0), float(np.max(np.abs(x1 - x0)))


def test_multigrid_histories_with_checkpoints_bitwise(mg):
    """the device-resident loop: the checkpoint variant of the fused kernel parks the decoded entries and re-uses them"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(2**16, p=3, pAgg=1, ratios=(4, 2, 2))
    b = U.rhs()
    N = len(b)
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        res = []
        for every in (1, 3):
            x, it, r = mg.multigrid_dev(H, ctx.to_device(np.zeros(N)), ctx.to_device(b), 9, 1e-30, check_every=every)
            res.append((x.download(), it, list(r)))
        out.append(res)
        H.free()
    for (x1, it1, r1), (x0, it0, r0) in zip(*out):
        assert it1 == it0 and r1 == r0
        assert np.array_equal(x1, x0)


def test_residual_entry_point_bitwise(mg):
    """aggmg_residual on the fine operator (a launch with no sweeps: the coupling's mirror is read for the residual
    alone)"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    U = UniformDgAggHierarchy(2**14, p=3, pAgg=1, ratios=(4, 2, 2))
    b = U.rhs()
    u = np.random.default_rng(1).standard_normal(len(b))
    out = []
    for on in (True, False):
        ctx = _ctx(mg, on)
        H = build_device_hierarchy(U, ctx)
        out.append((mg.residual(H._ops[0], u, b), H.sym_residual_levels()))
        H.free()
    (r1, lv1), (r0, lv0) = out
    assert lv1 == [0] and lv0 == []
    assert np.array_equal(r1, r0)
    A = U.stiffness_csc(0)
    assert np.allclose(r1, b - A @ u, rtol=0, atol=1e-9 * np.max(np.abs(b - A @ u)))


def _rank(rank, world, port, n, on, q):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    os.environ["AGGMG_SYM_RESIDUAL"] = "1" if on else "0"   # the default of every context this process creates
    import torch
    import torch.distributed as dist
    import agglomerationmultigrid1d_amd as mg
    from agglomerationmultigrid1d_amd import distributed as D
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ratios, p = (4, 2, 2), 3
        ctx = mg.Context(0)
        comm = D.Comm(world, rank, staged=True)
        layout = D.RankLayout(n, ratios, [p + 1, 2, 2, 2], world, rank)
        engine, U = D.build_local_uniform(n, p, 1, ratios, layout, ctx, comm)
        levels = engine.H.sym_residual_levels()
        dv = D.DistributedVCycle(engine, layout, comm)
        b = torch.from_numpy(U.rhs()).to(engine.dev)
        x = engine.new(layout.local_dofs(0))
        y = engine.new(layout.local_dofs(0))
        for _ in range(3):
            dv.vcycle(x, b, y)
            x, y = y, x
        torch.cuda.synchronize()
        q.put((rank, x.cpu().numpy()[layout.owned_slice(0)].copy(), levels))
    finally:
        dist.destroy_process_group()


def test_two_ranks_partitioned_bitwise(mg):
    """one element-partitioned cycle on 2 ranks: a rank's local arrays start with a ghost element whose coupling has
    no mirror in them (escape); owned rows equal the single-GPU cycle, option on or off"""
    import torch.multiprocessing as tmp
    from test_distributed_cpu import free_port
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy
    n = 2048
    U = UniformDgAggHierarchy(n, p=3, pAgg=1, ratios=(4, 2, 2))
    xs, _, _ = _cycles(mg, U, False, 3)
    got = {}
    for on in (True, False):
        sp = tmp.get_context("spawn")
        q = sp.Queue()
        port = free_port()
        procs = [sp.Process(target=_rank, args=(r, 2, port, n, on, q)) for r in range(2)]
        for pr in procs:
            pr.start()
        res = sorted((q.get(timeout=600) for _ in range(2)), key=lambda t: t[0])
        for pr in procs:
            pr.join(600)
        assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
        got[on] = res
    for rank in range(2):
        assert got[True][rank][2] == [0] and got[False][rank][2] == [], (got[True][rank][2], got[False][rank][2])
        assert np.array_equal(got[True][rank][1], got[False][rank][1])
    assert np.array_equal(np.concatenate([got[True][0][1], got[True][1][1]]), xs)
