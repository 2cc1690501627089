"""The element-partitioned cycle on meshes with unequal elements (tests/test_distributed_nonuniform_cpu.py,
tests/test_gpu_distributed_nonuniform.py).

Every other test of the partitioned path builds its operators with the library's uniform generator, rank by rank
(build_local_uniform -> UniformDgAggHierarchy(elem_range=)): every interior element of a level has the same record bit
for bit, so an operator, inverse block or transfer read at the wrong element offset -- a rank's offset, a tile subset of
the split ascent, a block range of the chunked coarsest solve, the rank order of the gathered coarsest block rows --
gives the right bits.  Here a rank's operators are SLICES of one global oracle hierarchy on a jittered
(jitter_helpers) or periodic (periodic_helpers) mesh: the local hierarchy of a rank is the principal sub-hierarchy of
the global one on layout.loc[k] -- rows and columns loc[k] of mStiffness[k], rows loc[k] by columns loc[k + 1] of
mInterpolation[k] -- which is what elem_range means ("couplings to elements outside the range are dropped, everything
else equals the corresponding entries of the global operators").

build_local_engine follows distributed.build_local_uniform step for step with the sliced matrices in place of the
generator's; the coarsest operator is gathered from the ranks' owned block rows by the library's own
distributed.gathered_coarse_hierarchy.  Called with a one-rank layout it builds the single-GPU hierarchy the same way.

shifted_operators is the control: one rank reads the sub-hierarchy of a range moved by whole coarsest-level elements,
what an offset error in the library would amount to."""
import contextlib
import threading

import numpy as np
import scipy.sparse as sp

import jitter_helpers as jh
import periodic_helpers as ph

_SHIFT = {}      # rank -> shift in coarsest-level elements, while shifted_operators is open

DICTIONARY_CAP = 1024        # records a level's operator dictionary holds at most (kDictMaxClasses, csrc/setup.hip)


def case_of(case):
    for cases in (jh.CASES, ph.CASES):
        if case in cases:
            return cases[case]
    raise KeyError(case)


def shape_of(case):
    """-> (n, ratios, block sizes) of a jitter_helpers / periodic_helpers case"""
    n, p, pAgg, nAgg, first = case_of(case)[:5]
    return n, (first,) + (2,) * (nAgg - 1), [p + 1] + [pAgg + 1] * nAgg


def build(oracle, case, nonuniform=True):
    """-> (Ho, b): the oracle's hierarchy and right-hand side of a case, on its non-uniform or on the uniform mesh"""
    if case in jh.CASES:
        return jh.build(oracle, case, nonuniform)
    return ph.build(oracle, case, nonuniform)


def thread_ranks(world, fn, limit=240, fault=None, device_errors=()):
    """fn(rank, comm) on `world` <= 8 ThreadComm ranks (threads of this process) -> list of results by rank.  Every
    thread is joined for at most `limit` seconds; a rank still alive then fails the call (and is recorded in `fault`, a
    list a GPU module keeps so that nothing more of it starts), as does a rank's exception -- recorded in `fault` too
    when its traceback holds one of `device_errors`."""
    from agglomerationmultigrid1d_amd import distributed as D
    assert world <= 8
    g = D.ThreadGroup(world)
    out, errs = [None] * world, []

    def one(r):
        try:
            out[r] = fn(r, D.ThreadComm(g, r))
        except BaseException:
            import traceback
            errs.append((r, traceback.format_exc()))
            g.barrier.abort()

    ts = [threading.Thread(target=one, args=(r,), daemon=True) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(limit)
    hung = [r for r, t in enumerate(ts) if t.is_alive()]
    if hung:
        g.barrier.abort()
        if fault is not None:
            fault.append("a rank did not finish within its time limit")
    elif errs and fault is not None and any(k in errs[0][1] for k in device_errors):
        fault.append("a library call failed on the device")
    assert not hung, f"ranks {hung} did not finish within {limit} s"
    assert not errs, errs[0][1]
    return out


class Slices:
    """A[k]: local CSC operators, L[k]: local CSC transfers, inds[k]: contiguous 1-based mBlockInds (m x ne_local) of
    the smoothed levels, ranges[k]: the element range of level k that was read"""

    def __init__(self, A, L, inds, ranges):
        self.A, self.L, self.inds, self.ranges = A, L, inds, ranges


def _contiguous_inds(m, ne):
    return np.arange(ne, dtype=np.int64)[None, :] * m + np.arange(1, m + 1, dtype=np.int64)[:, None]


def read_ranges(layout):
    """the element range slice_local reads on every level: layout.loc[k], moved while shifted_operators is open for the
    layout's rank (only where the moved range stays inside the level)"""
    shift = _SHIFT.get(layout.rank, 0)
    out = []
    for k, (lo, hi) in enumerate(layout.loc):
        s = shift * int(np.prod(layout.ratios[k:], dtype=np.int64))
        if shift and 0 <= lo + s and hi + s <= layout.ne[k]:
            lo, hi = lo + s, hi + s
        out.append((lo, hi))
    return out


def slice_local(Ho, layout):
    """-> Slices: the principal sub-hierarchy of the oracle DG hierarchy Ho on the layout's local element ranges"""
    nl = len(Ho.mStiffness)
    assert nl == len(layout.m) == len(layout.loc)
    for k in range(nl):
        assert Ho.mStiffness[k].shape[0] == layout.ne[k] * layout.m[k], (k, Ho.mStiffness[k].shape, layout.ne[k], layout.m[k])
    for k in range(nl - 1):      # element-contiguous unknowns: element e holds rows e m .. (e + 1) m - 1
        assert np.array_equal(np.asarray(Ho.mSmoothers[k].mBlockInds), _contiguous_inds(layout.m[k], layout.ne[k])), k
    rng = read_ranges(layout)
    rows = [slice(lo * layout.m[k], hi * layout.m[k]) for k, (lo, hi) in enumerate(rng)]
    A, L = [], []
    for k in range(nl):
        a = sp.csc_matrix(Ho.mStiffness[k])[rows[k], rows[k]].tocsc()
        a.sort_indices()
        A.append(a)
        if k < nl - 1:
            t = sp.csc_matrix(Ho.mInterpolation[k])[rows[k], rows[k + 1]].tocsc()
            t.sort_indices()
            L.append(t)
    inds = [_contiguous_inds(layout.m[k], rng[k][1] - rng[k][0]) for k in range(nl - 1)]
    return Slices(A, L, inds, rng)


def diagonal_blocks(A, m):
    """the m x m diagonal blocks of a CSC / CSR operator with element-contiguous unknowns -> (ne, m, m)"""
    ne = A.shape[0] // m
    C = sp.csr_matrix(A)
    return np.stack([C[e * m:(e + 1) * m, e * m:(e + 1) * m].toarray() for e in range(ne)])


class _Ref:
    pass


def local_ref(oracle, Ho, layout, gs=False):
    """the reference's field names (as dist_helpers.LocalRef) on the sliced operators, block-Jacobi smoothers factored
    from the sliced operators' own diagonal blocks (gs: the oracle's red-black block Gauss-Seidel on the same blocks)"""
    S = slice_local(Ho, layout)
    R = _Ref()
    n = len(S.A)
    R.mMeshes = [None] * n
    R.mStiffness, R.mInterpolation = S.A, S.L
    cls = oracle.BlockGaussSeidelRB if gs else oracle.BlockJacobi
    R.mSmoothers = [cls([oracle.LU(B) for B in diagonal_blocks(S.A[k], layout.m[k])], S.inds[k]) for k in range(n - 1)]
    R.ranges = S.ranges
    return R


def owned_coarse_block_rows(S, layout):
    """-> (sub, diag, sup), each (owned blocks, m, m): the blocks (e, e - 1), (e, e), (e, e + 1) of the rank's OWNED
    coarsest elements from its local coarsest operator (a first / last owned row couples to a ghost column that exists
    locally unless the rank sits at the domain boundary, where the block is zero)"""
    nc = len(S.A) - 1
    m = layout.m[nc]
    gl, _ = layout.ghosts(nc)
    no = layout.own[nc][1] - layout.own[nc][0]
    D = S.A[nc].toarray()
    nloc = D.shape[0] // m
    out = np.zeros((3, no, m, m))
    for i in range(no):
        e = gl + i
        for j, c in enumerate((e - 1, e, e + 1)):
            if 0 <= c < nloc:
                out[j, i] = D[e * m:(e + 1) * m, c * m:(c + 1) * m]
    return out[0], out[1], out[2]


def build_local_engine(mg, D, Ho, layout, ctx, comm, smoother="blockJac"):
    """distributed.build_local_uniform with the slices of Ho in place of the uniform generator's matrices:
    DeviceOperator uploads, the smoother of every level through the same `make`, MeshHierarchy(descriptors, ops, sms,
    Ls, keep_host=False, coarse_mode=COARSE_EXTERNAL) with uniform.LevelDescriptor, the coarsest operator gathered from
    every rank's owned block rows through the communicator (distributed.gathered_coarse_hierarchy) -> HipEngine.
    A one-rank layout (the whole range): the same construction with COARSE_AUTO -> the single-GPU MeshHierarchy."""
    from agglomerationmultigrid1d_amd import _lib
    from agglomerationmultigrid1d_amd.uniform import LevelDescriptor
    S = slice_local(Ho, layout)
    nl = len(S.A)
    kinds = D.smoother_kinds(smoother, nl - 1)
    if smoother not in ("blockJac", "blockGS") and layout.world > 1:
        need = D.halo_widths(layout.ratios, layout.nPre, layout.nPost, smoothers=kinds)
        assert all(w >= v for w, v in zip(layout.W, need)), (layout.W, need)

    def make(kind, op, inds):
        if kind == "patchSchwarz":
            return mg.ElementPatchSchwarz(op, inds.shape[0], inds.shape[1], ctx=ctx)
        if kind == "patchGS":
            return mg.ElementPatchGaussSeidel(op, inds.shape[0], inds.shape[1], ctx=ctx)
        return {"blockJac": mg.BlockJacobi, "blockGS": mg.BlockGaussSeidel}[kind](op, inds, ctx)

    ops, sms = [], []
    for k in range(nl):
        op = mg.DeviceOperator(S.A[k], _lib.OP_STIFFNESS, ctx)
        ops.append(op)
        if k < nl - 1:
            sms.append(make(kinds[k], op, S.inds[k]))
    Ls = [mg.DeviceOperator(S.L[k], _lib.OP_TRANSFER, ctx) for k in range(nl - 1)]
    desc = [LevelDescriptor(layout.m[k] - 1, S.ranges[k][1] - S.ranges[k][0]) for k in range(nl)]
    whole = layout.world == 1
    H = mg.MeshHierarchy(desc, ops, sms, Ls, ctx=ctx, keep_host=False,
                         coarse_mode=_lib.COARSE_AUTO if whole else _lib.COARSE_EXTERNAL)
    if whole:
        return H
    Hc = D.gathered_coarse_hierarchy(*owned_coarse_block_rows(S, layout), ctx, comm)
    return D.HipEngine(H, Hc, ctx)


@contextlib.contextmanager
def shifted_operators(layout, rank, shift):
    """while open, slice_local reads, for `rank`, the ranges of loc[k] moved by shift * prod(ratios[k:]) elements (whole
    coarsest-level elements, so that the moved hierarchy is still a nested one) -- where the moved range stays inside
    the level.  `layout`: that rank's layout; the move must apply on every level of it."""
    assert layout.rank == rank and rank not in _SHIFT
    _SHIFT[rank] = int(shift)
    try:
        assert all(a != b for a, b in zip(read_ranges(layout), layout.loc)), "the moved range leaves the level"
        yield
    finally:
        del _SHIFT[rank]


def local_vector(layout, v, level=0):
    """the local part (owned + ghosts) of a global level vector"""
    lo, hi = layout.loc[level]
    m = layout.m[level]
    return np.array(v[lo * m:hi * m])


def poisoned_ghosts(layout, v):
    """local_vector with the ghost entries overwritten by 123 (left) / -321 (right): the exchange must repair them"""
    x = local_vector(layout, v)
    sl = layout.owned_slice(0)
    x[:sl.start] = 123.0
    x[sl.stop:] = -321.0
    return x
