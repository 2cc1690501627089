"""Meshes with unequal elements under a uniform agglomeration ratio, for the tests of the uniform-ratio fused kernels
(tests/test_jitter_sensitivity_cpu.py, tests/test_gpu_jittered_uniform_ratio.py).

On a uniform mesh every interior element of a level has the same operator record, inverse block and transfer block, so a
kernel that loads a neighbour's record computes the same answer.  Here every interior vertex is moved by a seeded +-0.3
of the element width (the mesh of tests/test_gpu_chain_multi.py::test_jittered_mesh_columns_bitwise) while the
agglomerates keep one size per level: every element's record is its own, and the device still finds one ratio in the
transfer's structure.

The three mutations are the index errors such a kernel could make, made on the oracle's own arrays at one interior
element of one level: the right-hand neighbour's inverse block, transfer block or operator block row in place of the
element's own.  The CPU test shows that each moves the oracle's cycle far above the GPU tests' tolerance on the jittered
mesh and not at all on the uniform one."""
import contextlib

import numpy as np
import scipy.sparse as sp

# (n, p, pAgg, nAgg, first): oracle.build_dg_agg_hierarchy's arguments
CASES = {
    "c34": (2048, 3, 1, 3, 4),        # the config 3/4 shape: about 19 fine tiles; levels 1, 2 of 512, 256 elements
    "c34_small": (768, 3, 1, 3, 4),   # every level within a dictionary's 1024 records
    "b2": (2048, 1, 0, 4, 2),         # block size 2, one coarse row per agglomerate, ratios 2:2:2:2
    "p2": (1536, 2, 1, 3, 4),         # n no power of two, block size 3
    "b8": (1024, 7, 1, 2, 4),         # block size 8
}
ALPHA = 2.0 / 3.0
NCYC = 4                 # cycles of the loops
MULTI_CASES = ("c34", "b2")   # the cases of the K-column tests
MULTI_SEED = 40
X0_SEED = 11             # the first iterate of the one-cycle tests: splitmix_normal(N, X0_SEED)
RESIDUAL_TOL = 1e-12     # ||A (x - x_ref)|| <= RESIDUAL_TOL (||b|| + ||A x0||), tests/test_gpu_random_shapes.py
ITERATE_TOL = 1e-10      # ||x - x_ref|| <= ITERATE_TOL ||x_ref||, tests/test_gpu_pair.py
# (Reference against reference, sparse against dense LU at the coarsest level, from the first iterate of X0_SEED: at most
# 2.1e-11 at V(3,3), 1.2e-11 at c34's other sweep counts.  The iterate feels the coarsest solve's conditioning, the residual
# does not: from the first iterate of seed 3 the reference differs from itself by 1.35e-10 at V(0,3), 4.7e-15 in the residual.)


def loop_iterate_tol(cycle):
    """the bound on the iterate after `cycle` V(3,3) cycles from a zero first iterate: 1e-10 after the first, as
    tests/test_gpu_pair.py (reference against reference here: at most 2.4e-11).  From the second cycle on the reference
    differs from itself by up to 3.6e-10 (b8, third cycle; c34 2.4e-10) while its residuals agree to 4.7e-15 ||b||: the
    difference sits in the smoothest modes, which the operator hardly sees.  Ten times the reference's own figure."""
    return ITERATE_TOL if cycle == 1 else 4e-9


def columns(oracle, b, K, seed):
    """K right-hand sides and first iterates: b, -b / 2, then seeded normal vectors; seeded normal first iterates, all
    distinct.  (Entries of size one.  A random right-hand side of the size of ||b||, which the boundary penalty makes
    1e6, has a solution whose round-off in the coarsest solve alone is 8e-11 of the scale, reference against
    reference; with these columns that figure is at most 6.8e-15.)"""
    N = len(b)
    B = np.column_stack([b, -0.5 * b] + [oracle.splitmix_normal(N, seed + j) for j in range(2, K)])[:, :K]
    X0 = np.column_stack([oracle.splitmix_normal(N, seed + 100 + j) for j in range(K)])
    return B, X0


@contextlib.contextmanager
def jittered_mesh(oracle, amplitude=0.3, seed=5):
    """oracle.create_uniform_mesh moves every interior vertex by a seeded +-amplitude of the element width while this
    is open; the oracle's builders take their mesh from it (model_problem)"""
    uniform = oracle.create_uniform_mesh

    def jittered(n_, xin, xout):
        mesh = uniform(n_, xin, xout)
        d = np.random.default_rng(seed).uniform(-amplitude, amplitude, n_ + 1) * (xout - xin) / n_
        for v, dv in zip(mesh.mVertices[1:-1], d[1:-1]):
            v.mX += dv
        return mesh

    oracle.create_uniform_mesh = jittered
    try:
        yield
    finally:
        oracle.create_uniform_mesh = uniform


def build(oracle, case, jitter):
    """-> (Ho, b): the oracle's hierarchy and right-hand side of CASES[case], on the jittered or the uniform mesh"""
    n, p, pAgg, nAgg, first = CASES[case]
    with (jittered_mesh(oracle) if jitter else contextlib.nullcontext()):
        return oracle.build_dg_agg_hierarchy(n, p=p, pAgg=pAgg, nAgg=nAgg, first=first)


def smoothed_levels(Ho):
    return range(len(Ho.mStiffness) - 1)


def interior_element(Ho, k):
    """an element of level k with two neighbours on its right, away from both ends of the level"""
    ne = Ho.mSmoothers[k].mBlockInds.shape[1]
    assert ne >= 8
    return ne // 3


def _rows(Ho, k, e):
    """0-based unknowns of element e of level k"""
    return Ho.mSmoothers[k].mBlockInds[:, e] - 1


# ---- the mutations: context managers, the hierarchy is the oracle's own again on exit --------------------------------------
@contextlib.contextmanager
def neighbour_inverse_block(Ho, k, e=None):
    """mSmoothers[k].mBlocks[e] <- the block of element e + 1: the smoother solves with the neighbour's diagonal block"""
    e = interior_element(Ho, k) if e is None else e
    blocks = Ho.mSmoothers[k].mBlocks
    own = blocks[e]
    blocks[e] = blocks[e + 1]
    try:
        yield
    finally:
        blocks[e] = own


@contextlib.contextmanager
def neighbour_transfer_block(Ho, k, e=None):
    """mInterpolation[k]: the block of the agglomerate holding element e of level k <- the block of the agglomerate on
    its right (fine rows and coarse columns of an agglomerate read from the transfer's own pattern)"""
    e = interior_element(Ho, k) if e is None else e
    own = Ho.mInterpolation[k]
    L = sp.csc_matrix(own)
    rho = Ho.mSmoothers[k].mBlockInds.shape[1] // Ho.mSmoothers[k + 1].mBlockInds.shape[1]
    j = e // rho

    def block(jj):
        cols = _rows(Ho, k + 1, jj)
        rows = np.unique(L[:, cols].indices)
        return rows, cols

    (r0, c0), (r1, c1) = block(j), block(j + 1)
    assert len(r0) == len(r1) == rho * Ho.mSmoothers[k].mBlockInds.shape[0] and r0[-1] < r1[0]
    M = L.tolil()
    M[np.ix_(r0, c0)] = L[np.ix_(r1, c1)].toarray()
    Ho.mInterpolation[k] = M.tocsc()
    try:
        yield
    finally:
        Ho.mInterpolation[k] = own


@contextlib.contextmanager
def neighbour_operator_row(Ho, k, e=None):
    """mStiffness[k]: the block row of element e (its couplings to e - 1, e, e + 1) <- the block row of element e + 1
    (its couplings to e, e + 1, e + 2)"""
    e = interior_element(Ho, k) if e is None else e
    own = Ho.mStiffness[k]
    A = sp.csc_matrix(own)
    M = A.tolil()
    for d in (-1, 0, 1):
        M[np.ix_(_rows(Ho, k, e), _rows(Ho, k, e + d))] = A[np.ix_(_rows(Ho, k, e + 1), _rows(Ho, k, e + 1 + d))].toarray()
    Ho.mStiffness[k] = M.tocsc()
    try:
        yield
    finally:
        Ho.mStiffness[k] = own


MUTATIONS = {"smoother": neighbour_inverse_block, "transfer": neighbour_transfer_block, "operator": neighbour_operator_row}


def cycle_scale(Ho, b, x0):
    """||b|| + ||A x0||: the scale of tests/test_gpu_random_shapes.py's bound"""
    return float(np.linalg.norm(b) + (np.linalg.norm(Ho.mStiffness[0] @ x0) if x0 is not None else 0.0))


def dense_coarse_solve(A, rhs):
    """the coarsest solve by dense LU: the second reference of the reference-against-reference figures"""
    return np.linalg.solve(A.toarray(), np.asarray(rhs, dtype=np.float64))
