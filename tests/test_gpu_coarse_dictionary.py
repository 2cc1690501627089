"""The coarsest solve's dictionary (AGGMG_OPT_COARSE_DICTIONARY; csrc/cr_kernels.hpp: cr_stage_forward_dict_kernel,
cr_stage_backward_dict_kernel; csrc/setup.hip: setup_cr_dictionary): a chunk stage whose levels hold few distinct factor
records keeps them in LDS and reads them by class.  Every case compares, as 64-bit patterns, a hierarchy created with the
option on against one created with it off in the same context, and asserts which kernels ran: the counter
aggmg_coarse_dictionary_launches grows by two per stage that took the form and solve (once per column group), and not
at all with the option off; aggmg_hier_coarse_dictionary names the stages.

The helper system is block-tridiagonal Toeplitz with changed first and last diagonal blocks: its reduction levels have a
handful of distinct rows each (asserted: at most 8 classes per level and kind), whatever the size.  AGGMG_CR_TAIL_ROWS /
AGGMG_CR_MAX_Q shrink the tail and the chunks as in tests/test_gpu_coarse_cr.py, so that small systems run several
stages."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as m
    return m


@pytest.fixture(scope="module")
def ctx(mg):
    return mg.Context(0)


def toeplitz(nb, m, seed=1):
    """block-tridiagonal Toeplitz, not symmetric, block-diagonally dominant; the first and the last diagonal block differ"""
    rng = np.random.default_rng(seed)
    D, Lo, Up, D0, D1 = (rng.standard_normal((m, m)) for _ in range(5))
    diag = np.broadcast_to(D + 4.0 * m * np.eye(m), (nb, m, m)).copy()
    diag[0] += D0 + m * np.eye(m)
    diag[-1] += D1 + 2.0 * m * np.eye(m)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dr, dc, blk in ((0, 0, diag), (1, 0, np.broadcast_to(Lo, (nb - 1, m, m))), (0, 1, np.broadcast_to(Up, (nb - 1, m, m)))):
        e = np.arange(blk.shape[0])
        rows.append(((e + dr)[:, None, None] * m + ii).ravel())
        cols.append(((e + dc)[:, None, None] * m + jj).ravel())
        vals.append(np.ascontiguousarray(blk).ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nb * m, nb * m))


def random_blocks(nb, m, seed):
    """every row a class of its own (tests/test_gpu_coarse_cr.py: block_tridiag)"""
    rng = np.random.default_rng(seed)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dr, dc, cnt, shift in ((0, 0, nb, 4.0 * m), (1, 0, nb - 1, 0.0), (0, 1, nb - 1, 0.0)):
        blk = rng.standard_normal((cnt, m, m)) + shift * np.eye(m)
        e = np.arange(cnt)
        rows.append(((e + dr)[:, None, None] * m + ii).ravel())
        cols.append(((e + dc)[:, None, None] * m + jj).ravel())
        vals.append(blk.ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nb * m, nb * m))


def one_level(mg, ctx, A, cap):
    """the one-level hierarchy of A (its V-cycle with 0 sweeps is the direct solve), created under the option's value cap"""
    from agglomerationmultigrid1d_amd import _lib
    ctx.set_option(_lib.OPT_COARSE_DICTIONARY, cap)
    try:
        op = mg.DeviceOperator(A, _lib.OP_STIFFNESS, ctx)
        return mg.MeshHierarchy(None, [op], [], [], ctx=ctx, keep_host=False, coarse_mode=_lib.COARSE_DEVICE_CR)
    finally:
        ctx.set_option(_lib.OPT_COARSE_DICTIONARY, ctx.coarse_dictionary_cap()[1])


def solve(ctx, H, b):
    N = b.size
    x, z = ctx.alloc(N), ctx.to_device(np.zeros(N))
    H.vcycle_dev(z, ctx.to_device(b), x, 0, 0, 1.0)
    return x.download()


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


def counted(ctx, f):
    """(result of f(), launches the dictionary kernels served meanwhile)"""
    n0 = ctx.coarse_dictionary_launches()
    r = f()
    return r, ctx.coarse_dictionary_launches() - n0


def check_taken(H, m):
    """every stage took the form, with few classes on every level; -> the number of stages"""
    d = H.coarse_dictionary()
    assert d["stages"] and all(s["taken"] for s in d["stages"]), d
    assert all(1 <= c <= 8 for c in d["even_classes"] + d["odd_classes"]), d
    return len(d["stages"])


def test_option_values(mg, ctx):
    from agglomerationmultigrid1d_amd import _lib
    cap, top = ctx.coarse_dictionary_cap()
    assert cap == top == 56
    for bad in (-1, top + 1):
        with pytest.raises(Exception):
            ctx.set_option(_lib.OPT_COARSE_DICTIONARY, bad)
    assert ctx.coarse_dictionary_cap()[0] == top


@pytest.mark.parametrize("tail_rows,max_q", [(32, 4), (64, 5), (8, 12)])
@pytest.mark.parametrize("nb", [4096, 4099, 5000, (1 << 14) + 7])
@pytest.mark.parametrize("m", [1, 2])
def test_stage_shapes(mg, ctx, monkeypatch, m, nb, tail_rows, max_q):
    """a power of two, odd sizes whose levels end in clamped rows, a last chunk that is nearly empty; two or three stages,
    one stage of several steps"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A = toeplitz(nb, m)
    b = np.random.default_rng(nb + m).standard_normal(nb * m)
    Hoff = one_level(mg, ctx, A, 0)
    assert not any(s["taken"] for s in Hoff.coarse_dictionary()["stages"])
    xoff, n = counted(ctx, lambda: solve(ctx, Hoff, b))
    assert n == 0
    Hon = one_level(mg, ctx, A, 56)
    ns = check_taken(Hon, m)
    assert ns >= (1 if max_q == 12 else 2)
    xon, n = counted(ctx, lambda: solve(ctx, Hon, b))
    assert n == 2 * ns
    assert same_bits(xon, xoff)
    assert np.linalg.norm(A @ xon - b) <= 1e-12 * np.linalg.norm(b)
    x2, n = counted(ctx, lambda: solve(ctx, Hon, b))      # the same handle again
    assert n == 2 * ns and same_bits(x2, xon)
    Hoff.free()
    Hon.free()


def test_the_benchmark_operator(mg, ctx, monkeypatch):
    """the hierarchy bench.py runs, at 2^14 elements: its coarsest level has 1024 blocks of 2, which run stages under the
    knobs.  One V(3,3) cycle and three cycles back to back, bits on = bits off; the class counts stay under what the
    operator's structure gives at this size (at most 13 odd-row and 15 even-multiplier classes per level)"""
    from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy, build_device_hierarchy
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    from agglomerationmultigrid1d_amd import _lib
    U = UniformDgAggHierarchy(1 << 14, p=3, pAgg=1, ratios=(4, 2, 2))
    N = U.stiffness_csc(0).shape[0]
    b = np.random.default_rng(3).standard_normal(N)
    out = {}
    for cap in (0, 56):
        ctx.set_option(_lib.OPT_COARSE_DICTIONARY, cap)
        try:
            H = build_device_hierarchy(U, ctx=ctx)
        finally:
            ctx.set_option(_lib.OPT_COARSE_DICTIONARY, 56)
        d = H.coarse_dictionary()
        assert len(d["stages"]) >= 2, d
        z, bd, x1, x3 = ctx.to_device(np.zeros(N)), ctx.to_device(b), ctx.alloc(N), ctx.alloc(N)
        n0 = ctx.coarse_dictionary_launches()
        H.vcycle_dev(z, bd, x1)
        n1 = ctx.coarse_dictionary_launches()
        H.vcycles_dev(z, bd, x3, 3)
        n3 = ctx.coarse_dictionary_launches()
        out[cap] = (x1.download(), x3.download())
        if cap:
            assert all(s["taken"] for s in d["stages"]), d
            assert all(1 <= c <= 15 for c in d["even_classes"]) and all(1 <= c <= 13 for c in d["odd_classes"]), d
            assert n1 - n0 == 2 * len(d["stages"]) and n3 - n1 == 6 * len(d["stages"])
        else:
            assert not any(s["taken"] for s in d["stages"]) and n3 == n0
        H.free()
    assert same_bits(out[0][0], out[56][0]) and same_bits(out[0][1], out[56][1])


@pytest.mark.parametrize("m", [1, 2])
def test_over_the_cap(mg, ctx, monkeypatch, m):
    """random blocks, every row a class of its own: no stage takes the form, and the bits are those of the option off
    (tail and chunks such that the smallest level of a stage, 157 blocks, still has more even and odd rows than the cap)"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "256")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "3")
    nb = 5000
    A = random_blocks(nb, m, seed=9 + m)
    b = np.random.default_rng(4).standard_normal(nb * m)
    Hoff, Hon = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    d = Hon.coarse_dictionary()
    assert len(d["stages"]) >= 2 and not any(s["taken"] for s in d["stages"]), d
    xoff = solve(ctx, Hoff, b)
    xon, n = counted(ctx, lambda: solve(ctx, Hon, b))
    assert n == 0 and same_bits(xon, xoff)
    Hoff.free()
    Hon.free()


@pytest.mark.parametrize("m", [1, 2])
def test_at_the_cap(mg, ctx, monkeypatch, m):
    """the option's value equal to the largest class count: every stage takes the form; one less: the stage that holds
    that level does not"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    nb = 4099
    A = toeplitz(nb, m)
    b = np.random.default_rng(6).standard_normal(nb * m)
    H = one_level(mg, ctx, A, 56)
    d = H.coarse_dictionary()
    top = max(d["even_classes"] + d["odd_classes"])
    assert 2 <= top <= 8, d
    x = solve(ctx, H, b)
    H.free()
    Hat = one_level(mg, ctx, A, top)
    dat = Hat.coarse_dictionary()
    assert all(s["taken"] for s in dat["stages"]), dat
    xat, n = counted(ctx, lambda: solve(ctx, Hat, b))
    assert n == 2 * len(dat["stages"]) and same_bits(xat, x)
    Hat.free()
    Hbelow = one_level(mg, ctx, A, top - 1)
    db = Hbelow.coarse_dictionary()
    for s in db["stages"]:
        lv = range(s["first_level"], s["first_level"] + s["levels"])
        over = any(d["even_classes"][l] > top - 1 or d["odd_classes"][l] > top - 1 for l in lv)
        assert s["taken"] == (not over), (s, d)
    assert not all(s["taken"] for s in db["stages"])
    xb, n = counted(ctx, lambda: solve(ctx, Hbelow, b))
    assert n == 2 * sum(s["taken"] for s in db["stages"]) and same_bits(xb, x)
    Hbelow.free()


@pytest.mark.parametrize("m", [1, 2])
def test_k_columns(mg, ctx, monkeypatch, m):
    """K = 3 through the K-column cycle with 0 sweeps, in place (ld = N) and staged (ld = N + 3): every column has the
    single-column solve's bits, and a group costs the launches of one column"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    nb, K = 5000, 3
    A = toeplitz(nb, m)
    N = nb * m
    B = np.random.default_rng(8).standard_normal((N, K))
    Hoff, Hon = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    ns = check_taken(Hon, m)
    ref = np.column_stack([solve(ctx, Hoff, B[:, j]) for j in range(K)])
    for ld in (N, N + 3):
        pad = np.full((ld, K), np.nan, order="F")
        pad[:N] = B
        dB, dX = ctx.to_device(pad.ravel(order="F")), ctx.to_device(np.full(ld * K, np.nan))
        _, n = counted(ctx, lambda: Hon.vcycle_multi_dev(None, dB, dX, K, ld, nPre=0, nPost=0, alpha=1.0))
        got = dX.download().reshape((ld, K), order="F")
        assert n == 2 * ns
        for j in range(K):
            assert same_bits(got[:N, j], ref[:, j]), (ld - N, j)
        assert np.isnan(got[N:]).all()
    Hoff.free()
    Hon.free()


@pytest.mark.parametrize("nb,m,tail_rows,max_q", [(1 << 15, 1, 64, 5), ((1 << 14) + 7, 2, 32, 4)])
def test_partitioned_phases(mg, ctx, monkeypatch, nb, m, tail_rows, max_q):
    """cuts at thirds of the chunks through the phase entry points, as in tests/test_gpu_coarse_cr.py::test_cr_several_stages:
    the bits of the whole solve, with the option on"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A = toeplitz(nb, m)
    N = nb * m
    b = np.random.default_rng(2).standard_normal(N)
    Hoff, H = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    ns = check_taken(H, m)
    x = solve(ctx, Hoff, b)
    c = ctx
    q, nq, mb, nblk = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    c.check(c.lib.aggmg_coarse_plan(c.handle, H.handle, ctypes.byref(q), ctypes.byref(nq), ctypes.byref(mb), ctypes.byref(nblk)))
    assert 0 < q.value <= max_q and nq.value * m > tail_rows
    chunk = 1 << q.value
    nchunks = (nb + chunk - 1) // chunk
    cuts = [0, (nchunks // 3) * chunk, (2 * nchunks // 3) * chunk, nb]
    bd = ctx.to_device(b)
    partR, partL = ctx.to_device(np.zeros((nq.value + 1) * m)), ctx.to_device(np.zeros((nq.value + 1) * m))
    xq, out = ctx.alloc((nq.value + 1) * m), ctx.to_device(np.zeros(N))
    n0 = ctx.coarse_dictionary_launches()
    for r in range(3):
        c.check(c.lib.aggmg_coarse_chunk_forward_dev(c.handle, H.handle, bd.ptr.value + 8 * cuts[r] * m, cuts[r], cuts[r + 1],
                                                     partR.ptr, partL.ptr))
    c.check(c.lib.aggmg_coarse_boundary_solve_dev(c.handle, H.handle, partR.ptr, partL.ptr, xq.ptr))
    for r in range(3):
        c.check(c.lib.aggmg_coarse_chunk_backward_dev(c.handle, H.handle, bd.ptr.value + 8 * cuts[r] * m, cuts[r], cuts[r + 1],
                                                      xq.ptr, out.ptr.value + 8 * cuts[r] * m))
    assert ctx.coarse_dictionary_launches() - n0 == 6 + 2 * (ns - 1)      # stage 0 in three parts, the others whole
    assert same_bits(out.download(), x)
    Hoff.free()
    H.free()


def test_block_size_3_is_declined(mg, ctx, monkeypatch):
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    nb, m = 5000, 3
    A = toeplitz(nb, m)
    b = np.random.default_rng(12).standard_normal(nb * m)
    Hoff, Hon = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    assert Hon.coarse_info()["block_size"] == 3
    d = Hon.coarse_dictionary()
    assert d["stages"] and not any(s["taken"] for s in d["stages"]) and set(d["even_classes"] + d["odd_classes"]) == {-1}, d
    xoff = solve(ctx, Hoff, b)
    xon, n = counted(ctx, lambda: solve(ctx, Hon, b))
    assert n == 0 and same_bits(xon, xoff)
    Hoff.free()
    Hon.free()
