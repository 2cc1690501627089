"""The coarsest solve's dictionary (AGGMG_OPT_COARSE_DICTIONARY; csrc/cr_kernels.hpp: cr_stage_forward_dict_kernel,
cr_stage_backward_dict_kernel; csrc/setup.hip: setup_cr_dictionary): a chunk stage whose levels hold few distinct factor
records keeps them in LDS and reads them by class.  Every case compares, as 64-bit patterns, a hierarchy created with the
option on against one created with it off in the same context, and asserts which kernels ran: the counter
aggmg_coarse_dictionary_launches grows by two per stage that took the form and solve (once per column group), and not
at all with the option off; aggmg_hier_coarse_dictionary names the stages.

The helper system is block-tridiagonal Toeplitz with changed first and last diagonal blocks: its reduction levels have a
handful of distinct rows each (asserted: at most 8 classes per level and kind), whatever the size.  AGGMG_CR_TAIL_ROWS /
AGGMG_CR_MAX_Q shrink the tail and the chunks as in tests/test_gpu_coarse_cr.py, so that small systems run several
stages.

On that system every interior row of every reduction level is ONE class and all chunks but the first and the last carry
the same index arrays: a class index read at the wrong place -- the offset arithmetic of cr_pre_load_dict /
cr_pre_load_b_dict, the chunk offset c = c0 + blockIdx.x of the partitioned entry points, the chunk-major layout that
cr_dict_chunk_index_kernel writes -- gives the same bits but at the two ends, and with at most 8 classes per level the
table never outgrows the first rounds of cr_dict_fill.  The *_periodic tests therefore run periodic_blocks: P random block
rows tiled with an odd period P.  Row j of the next reduction level is row 2 j + 1 of this one, so an odd period survives
every level (asserted: at least P classes of each kind on the first level of every stage), neighbouring rows are in
different classes and successive chunks of 2^q rows start at different phases.  Option on against option off as bits,
the launch counter, and ||A x - b|| <= 1e-12 ||b|| as before (a float64 sparse LU solve of the same systems:
at most 1.8e-16, tests/test_periodic_sensitivity_cpu.py::test_sparse_lu_meets_the_coarse_bound).
Measured on the device: ||A x - b|| / ||b|| at most 2.1e-16 (P = 3 and 7); at P = 3 up to 5 even-row and 4 odd-row
classes per level, at P = 7 up to 9 and 8 (fewer on the last levels, of a few rows each), every stage taken.  The
table-remainder case (m = 2, P = 13, 2^14 + 7 blocks, one stage of 12 levels): 15 even and 13 or 14 odd classes on
levels 0 .. 8, fewer below, a table of 1632 16-byte words against the 6 x 256 = 1536 of the first rounds -- P = 13
reaches it and was not raised."""
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


def periodic_blocks(nb, m, P, seed):
    """P random block rows (diagonal, sub, super), not symmetric, block-diagonally dominant, tiled with the odd period P:
    row j has the blocks of row j mod P; the first and the last diagonal block differ as in toeplitz"""
    assert P % 2 == 1
    rng = np.random.default_rng(seed)
    D, Lo, Up = (rng.standard_normal((P, m, m)) for _ in range(3))
    D0, D1 = (rng.standard_normal((m, m)) for _ in range(2))
    e = np.arange(nb)
    diag = D[e % P] + 4.0 * m * np.eye(m)
    diag[0] += D0 + m * np.eye(m)
    diag[-1] += D1 + 2.0 * m * np.eye(m)
    ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = [], [], []
    for dr, dc, blk in ((0, 0, diag), (1, 0, Lo[e[1:] % P]), (0, 1, Up[e[:-1] % P])):
        k = np.arange(blk.shape[0])
        rows.append(((k + dr)[:, None, None] * m + ii).ravel())
        cols.append(((k + dc)[:, None, None] * m + jj).ravel())
        vals.append(np.ascontiguousarray(blk).ravel())
    return sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nb * m, nb * m))


def periodic_system(nb, m, P):
    """-> (A, b): the periodic system of a size, block size and period, and its right-hand side"""
    return periodic_blocks(nb, m, P, seed=100 * P + m), np.random.default_rng(nb + m + P).standard_normal(nb * m)


# (nb, m, P) of every periodic system below (the CPU test solves them by sparse LU)
STAGE_SYSTEMS = [(nb, m, P) for m in (1, 2) for P in (3, 7) for nb in (4099, 5000, (1 << 14) + 7)]
REMAINDER_SYSTEM = ((1 << 14) + 7, 2, 13)
PARTITIONED_SYSTEMS = [(1 << 15, 1, 7), ((1 << 14) + 7, 2, 7)]
COLUMN_SYSTEMS = [(5000, 1, 7), (5000, 2, 7)]
CAP_SYSTEMS = [(4099, 1, 7), (4099, 2, 7)]
PERIODIC_SYSTEMS = sorted(set(STAGE_SYSTEMS + [REMAINDER_SYSTEM] + PARTITIONED_SYSTEMS + COLUMN_SYSTEMS + CAP_SYSTEMS))


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


def check_periodic(H, P, what, nb, every_stage=True):
    """every stage took the form; at most 56 classes of each kind on every level, at least the period on the first level
    of every stage -- or as many as that level has rows of the kind, where a last stage begins on a level of fewer than
    2 P rows (level l has nb >> l rows: row j of the next level is row 2 j + 1); every_stage=False: on the first level of
    the first stage only; -> (the number of stages, the report)"""
    d = H.coarse_dictionary()
    print(f"[coarse periodic] {what}: stages {d['stages']} even classes {d['even_classes']} odd classes {d['odd_classes']}")
    assert d["stages"] and all(s["taken"] for s in d["stages"]), d
    assert all(1 <= c <= 56 for c in d["even_classes"] + d["odd_classes"]), d
    for s in d["stages"] if every_stage else ():
        l, rows = s["first_level"], nb >> s["first_level"]
        assert d["even_classes"][l] >= min(P, (rows + 1) // 2) and d["odd_classes"][l] >= min(P, rows // 2), (s, d)
    assert d["even_classes"][0] >= P and d["odd_classes"][0] >= P, d
    return len(d["stages"]), d


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


def _partitioned(mg, ctx, A, b, m, tail_rows, max_q, check):
    """cuts at thirds of the chunks through the three phase entry points against the whole solve with the option off"""
    nb, N = A.shape[0] // m, A.shape[0]
    Hoff, H = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    ns = check(H)
    x = solve(ctx, Hoff, b)
    c = ctx
    q, nq, mb, nblk = ctypes.c_int(0), ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int64(0)
    c.check(c.lib.aggmg_coarse_plan(c.handle, H.handle, ctypes.byref(q), ctypes.byref(nq), ctypes.byref(mb), ctypes.byref(nblk)))
    assert 0 < q.value <= max_q and nq.value * m > tail_rows
    chunk = 1 << q.value
    nchunks = (nb + chunk - 1) // chunk
    cuts = [0, (nchunks // 3) * chunk, (2 * nchunks // 3) * chunk, nb]
    assert 0 < cuts[1] < cuts[2] < nb
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
    return x


@pytest.mark.parametrize("nb,m,tail_rows,max_q", [(1 << 15, 1, 64, 5), ((1 << 14) + 7, 2, 32, 4)])
def test_partitioned_phases(mg, ctx, monkeypatch, nb, m, tail_rows, max_q):
    """cuts at thirds of the chunks through the phase entry points, as in tests/test_gpu_coarse_cr.py::test_cr_several_stages:
    the bits of the whole solve, with the option on"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A = toeplitz(nb, m)
    b = np.random.default_rng(2).standard_normal(nb * m)
    _partitioned(mg, ctx, A, b, m, tail_rows, max_q, lambda H: check_taken(H, m))


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


# ---- periodic systems: neighbouring rows in different classes, chunks that start at different phases ---------------------
@pytest.mark.parametrize("tail_rows,max_q", [(32, 4), (64, 5), (8, 12)])
@pytest.mark.parametrize("nb,m,P", STAGE_SYSTEMS, ids=[f"nb{nb}-m{m}-P{P}" for nb, m, P in STAGE_SYSTEMS])
def test_stage_shapes_periodic(mg, ctx, monkeypatch, nb, m, P, tail_rows, max_q):
    """test_stage_shapes on periodic systems: every stage taken, at least P classes of each kind on the first level of
    every stage, at most 56 on every level"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A, b = periodic_system(nb, m, P)
    Hoff = one_level(mg, ctx, A, 0)
    assert not any(s["taken"] for s in Hoff.coarse_dictionary()["stages"])
    xoff, n = counted(ctx, lambda: solve(ctx, Hoff, b))
    assert n == 0
    Hon = one_level(mg, ctx, A, 56)
    ns, _ = check_periodic(Hon, P, f"nb {nb} m {m} P {P} tail {tail_rows} max_q {max_q}", nb)
    assert ns >= (1 if max_q == 12 else 2)
    xon, n = counted(ctx, lambda: solve(ctx, Hon, b))
    assert n == 2 * ns
    res = float(np.linalg.norm(A @ xon - b) / np.linalg.norm(b))
    print(f"[coarse periodic] nb {nb} m {m} P {P} tail {tail_rows} max_q {max_q}: ||A x - b|| / ||b|| = {res:.3e}")
    assert same_bits(xon, xoff)
    assert res <= 1e-12
    x2, n = counted(ctx, lambda: solve(ctx, Hon, b))      # the same handle again
    assert n == 2 * ns and same_bits(x2, xon)
    Hoff.free()
    Hon.free()


def _table_double2(d, m):
    """the 16-byte words of every stage's table, from the reported class counts (host_plan.hpp: cr_dict_plan --
    even x cr_dict_even_words(m) + odd x cr_dict_odd_words(m) doubles per level)"""
    even_words, odd_words = 2 * m * m, (3 * m * m + (m + 1) // 2 + 1) & ~1
    return [sum(d["even_classes"][l] * even_words + d["odd_classes"][l] * odd_words
                for l in range(s["first_level"], s["first_level"] + s["levels"])) // 2 for s in d["stages"]]


def test_table_beyond_the_first_rounds_periodic(mg, ctx, monkeypatch):
    """a table of more than 6 x 256 16-byte words: cr_dict_fill copies the remainder in its loop, which no table of the
    Toeplitz system (at most 8 classes per level) reaches"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "8")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "12")
    nb, m, P = REMAINDER_SYSTEM
    A, b = periodic_system(nb, m, P)
    Hoff, Hon = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    # (a second stage of one level, 12, follows the 12 levels of the first: its 4 rows' multipliers have underflowed to
    # zero and are one class, so the period is asserted where the table is, on the first stage)
    ns, d = check_periodic(Hon, P, f"nb {nb} m {m} P {P} tail 8 max_q 12", nb, every_stage=False)
    words = _table_double2(d, m)
    print(f"[coarse periodic] table-remainder case: tables of {words} double2 words against 6 x 256 = 1536")
    assert max(words) > 6 * 256, (words, d)
    xoff = solve(ctx, Hoff, b)
    xon, n = counted(ctx, lambda: solve(ctx, Hon, b))
    res = float(np.linalg.norm(A @ xon - b) / np.linalg.norm(b))
    print(f"[coarse periodic] table-remainder case: ||A x - b|| / ||b|| = {res:.3e}")
    assert n == 2 * ns and same_bits(xon, xoff)
    assert res <= 1e-12
    Hoff.free()
    Hon.free()


@pytest.mark.parametrize("nb,m,P,tail_rows,max_q", [s + t for s, t in zip(PARTITIONED_SYSTEMS, [(64, 5), (32, 4)])])
def test_partitioned_phases_periodic(mg, ctx, monkeypatch, nb, m, P, tail_rows, max_q):
    """test_partitioned_phases where the chunks' index arrays differ, so that the chunk offset c0 of a part matters"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", str(tail_rows))
    monkeypatch.setenv("AGGMG_CR_MAX_Q", str(max_q))
    A, b = periodic_system(nb, m, P)
    x = _partitioned(mg, ctx, A, b, m, tail_rows, max_q, lambda H: check_periodic(H, P, f"partitioned nb {nb} m {m} P {P}", nb)[0])
    res = float(np.linalg.norm(A @ x - b) / np.linalg.norm(b))
    print(f"[coarse periodic] partitioned nb {nb} m {m} P {P}: ||A x - b|| / ||b|| = {res:.3e}")
    assert res <= 1e-12


@pytest.mark.parametrize("nb,m,P", COLUMN_SYSTEMS)
def test_k_columns_periodic(mg, ctx, monkeypatch, nb, m, P):
    """test_k_columns on a periodic system: every column has the single-column solve's bits"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    K = 3
    A, _ = periodic_system(nb, m, P)
    N = nb * m
    B = np.random.default_rng(8).standard_normal((N, K))
    Hoff, Hon = one_level(mg, ctx, A, 0), one_level(mg, ctx, A, 56)
    ns, _ = check_periodic(Hon, P, f"K columns nb {nb} m {m} P {P}", nb)
    ref = np.column_stack([solve(ctx, Hoff, B[:, j]) for j in range(K)])
    for j in range(K):
        res = float(np.linalg.norm(A @ ref[:, j] - B[:, j]) / np.linalg.norm(B[:, j]))
        print(f"[coarse periodic] K columns nb {nb} m {m} P {P} column {j}: ||A x - b|| / ||b|| = {res:.3e}")
        assert res <= 1e-12
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


@pytest.mark.parametrize("nb,m,P", CAP_SYSTEMS)
def test_at_the_cap_periodic(mg, ctx, monkeypatch, nb, m, P):
    """test_at_the_cap on a periodic system: the option at the largest class count takes every stage, one less declines
    exactly the stages that hold such a level; the same bits either way"""
    monkeypatch.setenv("AGGMG_CR_TAIL_ROWS", "32")
    monkeypatch.setenv("AGGMG_CR_MAX_Q", "4")
    A, b = periodic_system(nb, m, P)
    H = one_level(mg, ctx, A, 56)
    _, d = check_periodic(H, P, f"at the cap nb {nb} m {m} P {P}", nb)
    top = max(d["even_classes"] + d["odd_classes"])
    assert P <= top <= 56, d
    x = solve(ctx, H, b)
    res = float(np.linalg.norm(A @ x - b) / np.linalg.norm(b))
    print(f"[coarse periodic] at the cap nb {nb} m {m} P {P}: top {top}, ||A x - b|| / ||b|| = {res:.3e}")
    assert res <= 1e-12
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
