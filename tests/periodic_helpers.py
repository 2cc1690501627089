"""Periodic, strongly non-uniform meshes for the tests of the kernels that read the operator through a table of class
records in LDS (tests/test_periodic_sensitivity_cpu.py, tests/test_gpu_periodic_class_records.py): the fine level's
btd_elem_rec_kernel / btd_elem_rec_replay_up_kernel and the two-level btd_pair_down_elem_kernel / btd_pair_up_elem_kernel,
each of which takes a level of at most 32 distinct records.

On a uniform mesh every interior element of a level is in one class, so a class index read at the wrong place -- a
neighbour's, the previous tile's, a halo element's -- gives the same bits.  On the jittered meshes of
tests/jitter_helpers.py every element is a class of its own: every level is over the cap of 32 and those kernels never
run.  Here interior vertex i is moved by pattern[i % P] of the element width, with dyadic displacements and n a power of
two, so that every width is exact and the records repeat bit for bit: few classes (the LDS forms are taken), every
element's class different from both neighbours', successive tiles starting at different phases of the period.

input_classes is a host-side proxy of what the device's set-up counts; the device's own counts are asserted in the GPU
tests.  Distinct records per smoothed level (levels 0, 1, 2; elements 1024 / 256 / 128 at n = 1024, 512 / 128 / 64 at
n = 512), the same at both sizes:  period 3: 17 / 26 / 23;  period 5: 28 / 20 / 17  (uniform: 7 / 14 / 13 at n = 1024,
7 / 11 / 10 at n = 512).

The counts are this low only where the widths of a period are power-of-two multiples of one another or few: the
agglomerated operators are Galerkin products whose round-off depends on where an element lies, and with five unrelated
widths level 1 has 37 .. 61 records.  Period 5 with the two widths 5/4 and 5/8 (displacements 0, 1/4, -1/8, 1/8, -1/4 and
their rotations) has 21 .. 27 / 16 / 15 records, but an odd cycle of two widths has two equal neighbours somewhere, and every
rotation either starts two consecutive fine tiles in one class or hides one of the three index errors at the element
they are made at (change of the cycle 0 .. 9e-17).  The period-5 pattern here has the widths 5/2, 5/4, 5/8, 5/16, 5/16.

Tolerances, columns, mutations and cycle_scale are those of jitter_helpers.  Reference against reference (the oracle's
cycle with its sparse coarsest solve against dense LU there), measured on these meshes
(tests/test_periodic_sensitivity_cpu.py::test_reference_against_reference), largest figure of all cases:
 * ||A (x_dense - x_sparse)|| / scale: one cycle 7.2e-16, loops 7.9e-16, columns 4.3e-15: RESIDUAL_TOL = 1e-12 stands.
 * ||x_dense - x_sparse|| / ||x||, one cycle from the first iterate of X0_SEED and from none, at every sweep count:
   3.1e-11 (period 3: V(8,8) at n = 1024, V(1,2) at n = 512; period 5: 8.7e-13).  Ten times that is over jitter_helpers'
   ITERATE_TOL = 1e-10, so ten times the reference's own figure stands in: ONE_CYCLE_ITERATE_TOL = 4e-10.
 * the same after the first V(3,3) of a loop from zero: 1.3e-11; ten times that: loop_iterate_tol(1) = 2e-10.  After the
   later cycles: 1.2e-10; jitter_helpers.loop_iterate_tol's 4e-9 holds with a margin of 30.
 * the K-column tests' columns: 2.4e-13: ITERATE_TOL = 1e-10 stands (COLUMN_ITERATE_TOL).
 * ||A x_k - b|| of the two references: equal to 1.1e-13 relative, against the histories' rtol of 1e-8."""
import contextlib

import numpy as np
import scipy.sparse as sp

import jitter_helpers as jh

PATTERNS = {
    3: (0.0, 0.25, -0.125),                        # widths 5/4, 5/8, 9/8 of the uniform one
    5: (0.0625, 0.3125, -0.0625, -0.75, 0.75),     # widths 5/4, 5/8, 5/16, 5/2, 5/16 of the uniform one
}
# (n, p, pAgg, nAgg, first, period)
CASES = {
    "p3_1024": (1024, 3, 1, 3, 4, 3),   # about five element-thread tiles on level 0, two two-level descent tiles on level 2
    "p5_1024": (1024, 3, 1, 3, 4, 5),
    "p3_512": (512, 3, 1, 3, 4, 3),     # every level within one or two tiles
    "p5_512": (512, 3, 1, 3, 4, 5),
}
CAP = 32                  # kPairElemMaxClasses and the default of AGGMG_OPT_ELEMENT_RECORDS_LDS
FINE_TILE = 248           # elements a fine-level element-thread tile owns in the descent
SWEEPS = ((3, 3), (1, 2), (2, 3))
LONG_CASE, LONG_SWEEPS = "p3_1024", (8, 8)    # the largest halo the two-level launches take
MULTI_CASE, MULTI_K = "p5_1024", 3
ALPHA, NCYC, X0_SEED, MULTI_SEED = jh.ALPHA, jh.NCYC, jh.X0_SEED, jh.MULTI_SEED
RESIDUAL_TOL = jh.RESIDUAL_TOL
ONE_CYCLE_ITERATE_TOL = 4e-10        # ten times the reference's own 3.1e-11 (the module docstring)
COLUMN_ITERATE_TOL = jh.ITERATE_TOL


def loop_iterate_tol(cycle):
    """the bound on the iterate after `cycle` V(3,3) cycles from zero: ten times the reference's own 1.3e-11 after the
    first, jitter_helpers.loop_iterate_tol after the later ones (the module docstring)"""
    return 2e-10 if cycle == 1 else jh.loop_iterate_tol(cycle)


def sweeps_of(case):
    return SWEEPS + ((LONG_SWEEPS,) if case == LONG_CASE else ())


@contextlib.contextmanager
def periodic_mesh(oracle, pattern):
    """oracle.create_uniform_mesh moves interior vertex i by pattern[i % len(pattern)] of the element width while this is
    open (as jitter_helpers.jittered_mesh)"""
    uniform = oracle.create_uniform_mesh
    P = len(pattern)
    assert P % 2 == 1 and all(float(d * 64).is_integer() for d in pattern)
    assert all(1.0 + pattern[(i + 1) % P] - pattern[i] >= 0.25 for i in range(P)), "an element of under a quarter of the width"

    def periodic(n_, xin, xout):
        mesh = uniform(n_, xin, xout)
        h = (xout - xin) / n_
        for i, v in enumerate(mesh.mVertices):
            if 0 < i < n_:
                v.mX += pattern[i % P] * h
        return mesh

    oracle.create_uniform_mesh = periodic
    try:
        yield
    finally:
        oracle.create_uniform_mesh = uniform


def build(oracle, case, periodic=True):
    """-> (Ho, b): the oracle's hierarchy and right-hand side of CASES[case], on the periodic or the uniform mesh"""
    n, p, pAgg, nAgg, first, period = CASES[case]
    with (periodic_mesh(oracle, PATTERNS[period]) if periodic else contextlib.nullcontext()):
        return oracle.build_dg_agg_hierarchy(n, p=p, pAgg=pAgg, nAgg=nAgg, first=first)


def input_classes(Ho, k):
    """-> (number of distinct records of level k, the class of every element in order of first appearance).  An element's
    record: its sub, diagonal and super block of mStiffness[k], the float64 inverse of the diagonal block, its rows of
    mInterpolation[k]; two records are one class when all their bits agree"""
    inds = Ho.mSmoothers[k].mBlockInds - 1
    m, ne = inds.shape
    A = sp.csr_matrix(Ho.mStiffness[k])
    L = sp.csr_matrix(Ho.mInterpolation[k])
    zero = np.zeros((m, m))
    seen, seq = {}, []
    for e in range(ne):
        rows = inds[:, e]
        Ar = A[rows]
        sub = Ar[:, inds[:, e - 1]].toarray() if e > 0 else zero
        diag = Ar[:, rows].toarray()
        sup = Ar[:, inds[:, e + 1]].toarray() if e + 1 < ne else zero
        Lr = L[rows]
        transfer = Lr[:, np.unique(Lr.indices)].toarray()
        key = b"".join(np.ascontiguousarray(a + 0.0).tobytes() for a in (sub, diag, sup, np.linalg.inv(diag), transfer))
        seq.append(seen.setdefault(key, len(seen)))
    return len(seen), np.asarray(seq)
