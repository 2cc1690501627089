"""Why the class-record kernels are tested on periodic meshes (tests/test_gpu_periodic_class_records.py), shown with the
oracle alone on the meshes of tests/periodic_helpers.py.

 * Every smoothed level has at most 32 distinct records (the cap of both LDS forms), no element shares its class with
   either neighbour, and the first elements of consecutive fine tiles of 248 elements are in different classes.
 * One index error at one interior element of one level -- the right-hand neighbour's inverse block, transfer block or
   operator block row in place of the element's own (jitter_helpers.MUTATIONS) -- moves one V(3,3) from a random first
   iterate by at least 1e-10 scale, 100 times the 1e-12 scale the GPU tests allow (measured: 2.1e-7 at the least --
   the smoother error on level 2 of period 5, n = 512 -- and up to 1.1e+1, the smoother error on level 0 of period 5,
   n = 1024).
 * The reference against itself (sparse against dense LU at the coarsest level) at every sweep count, loop and column
   the GPU tests use: the figures of periodic_helpers' docstring, each asserted below a tenth of the GPU tests' bound.
 * The periodic systems of tests/test_gpu_coarse_dictionary.py, solved by sparse LU: ||A x - b|| <= 1.8e-16 ||b||, a
   margin of over a thousand under the 1e-12 those tests hold the device to."""
import numpy as np
import pytest

import jitter_helpers as jh
import periodic_helpers as ph

GPU_TOL = ph.RESIDUAL_TOL


@pytest.fixture(scope="module")
def built(oracle):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = ph.build(oracle, case)
        return cache[case]
    return get


@pytest.mark.parametrize("case", list(ph.CASES))
def test_few_classes_and_no_neighbour_alike(built, case):
    Ho, _ = built(case)
    period = ph.CASES[case][5]
    levels = list(jh.smoothed_levels(Ho))
    assert levels == [0, 1, 2]
    for k in levels:
        count, seq = ph.input_classes(Ho, k)
        alike = int(np.sum(seq[1:] == seq[:-1]))
        run = max(len(set(seq[i:i + 7].tolist())) for i in range(2, len(seq) - 9))
        print(f"[periodic] {case} level {k}: {len(seq)} elements, {count} classes, neighbours in one class {alike}, "
              f"distinct classes among 7 consecutive interior elements {run}")
        assert period <= count <= ph.CAP, (case, k, count)
        assert alike == 0, (case, k, alike)
        assert run == 7, (case, k, run)
    _, seq = ph.input_classes(Ho, 0)
    firsts = seq[::ph.FINE_TILE]
    print(f"[periodic] {case}: classes of the first elements of the fine tiles of {ph.FINE_TILE}: {firsts.tolist()}")
    assert len(firsts) >= 3 and np.all(firsts[1:] != firsts[:-1]), (case, firsts)


def test_the_uniform_mesh_has_one_interior_class(oracle):
    """the proxy on the uniform mesh of the first case's shape: 7 classes on the fine level (the device's own count,
    tests/test_gpu_elem_records.py): the first and the last element and, for the transfer's rows, the four places in an
    agglomerate -- every interior element is in the class of the element one agglomerate further"""
    Ho, _ = ph.build(oracle, "p3_512", periodic=False)
    count, seq = ph.input_classes(Ho, 0)
    print(f"[periodic] uniform n = 512, level 0: {count} classes")
    assert count == 7 and np.array_equal(seq[4:-8], seq[8:-4])


@pytest.mark.parametrize("case", list(ph.CASES))
def test_index_errors_show(oracle, built, case):
    Ho, b = built(case)
    x0 = oracle.splitmix_normal(len(b), ph.X0_SEED)
    A = Ho.mStiffness[0]
    scale = jh.cycle_scale(Ho, b, x0)
    x = oracle.multigrid_v_cycle(Ho, x0, b)
    for k in jh.smoothed_levels(Ho):
        moved = {}
        for name, mutate in jh.MUTATIONS.items():
            with mutate(Ho, k):
                xm = oracle.multigrid_v_cycle(Ho, x0, b)
            moved[name] = float(np.linalg.norm(A @ (xm - x))) / scale
        print(f"[periodic] {case} level {k} element {jh.interior_element(Ho, k)}: change of V(3,3) / scale  "
              + "   ".join(f"{name} {v:.2e}" for name, v in moved.items()))
        for name, v in moved.items():
            assert v >= 100.0 * GPU_TOL, (case, k, name, v)
    assert np.array_equal(oracle.multigrid_v_cycle(Ho, x0, b), x), "a mutation was not undone"


WORST = {}    # quantity -> the reference's largest difference from itself, printed by the last test


def _note(what, v):
    WORST[what] = max(WORST.get(what, 0.0), v)


@pytest.mark.parametrize("case", list(ph.CASES))
def test_reference_against_reference(oracle, built, case):
    """the residual figures are asserted below a tenth of the GPU tests' 1e-12, the iterate figures below a tenth of the
    bounds the GPU tests use (periodic_helpers' docstring has the measured figures)"""
    Ho, b = built(case)
    x0 = oracle.splitmix_normal(len(b), ph.X0_SEED)
    A = Ho.mStiffness[0]
    scale = jh.cycle_scale(Ho, b, x0)
    cycle = oracle.multigrid_v_cycle
    for x_first, what in ((x0, "one cycle"), (None, "one cycle, no first iterate")):
        start = np.zeros(len(b)) if x_first is None else x_first
        sc = jh.cycle_scale(Ho, b, x_first)
        for nPre, nPost in ph.sweeps_of(case):
            xs = cycle(Ho, start, b, nPre=nPre, nPost=nPost, alpha=ph.ALPHA)
            xd = cycle(Ho, start, b, nPre=nPre, nPost=nPost, alpha=ph.ALPHA, coarse_solve=jh.dense_coarse_solve)
            res = float(np.linalg.norm(A @ (xd - xs))) / sc
            rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
            print(f"[periodic] {case} V({nPre},{nPost}) {what}, reference against reference: residual {res:.2e} scale, iterate {rel:.2e}")
            _note(what + ": residual", res)
            _note(what + ": iterate", rel)
            assert res <= 0.1 * GPU_TOL and rel <= 0.1 * ph.ONE_CYCLE_ITERATE_TOL, (case, nPre, nPost, res, rel)
    assert scale > 0.0
    xs = xd = np.zeros(len(b))
    nb = float(np.linalg.norm(b))
    for cyc in range(1, ph.NCYC + 1):
        xs = cycle(Ho, xs, b)
        xd = cycle(Ho, xd, b, coarse_solve=jh.dense_coarse_solve)
        res = float(np.linalg.norm(A @ (xd - xs))) / nb
        rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
        rs, rd = float(np.linalg.norm(A @ xs - b)), float(np.linalg.norm(A @ xd - b))
        print(f"[periodic] {case} cycle {cyc} from zero, reference against reference: residual {res:.2e} ||b||, "
              f"iterate {rel:.2e}, ||A x - b|| {rs:.6e} / {rd:.6e}")
        _note("loop: residual", res)
        _note(f"loop: iterate, cycle {'1' if cyc == 1 else '2 on'}", rel)
        _note("loop: ||A x - b|| relative", abs(rd - rs) / rs)
        assert res <= 0.1 * GPU_TOL and rel <= 0.1 * ph.loop_iterate_tol(cyc), (case, cyc, res, rel)
        assert np.isclose(rd, rs, rtol=1e-9, atol=1e-12 * nb), (case, cyc, rs, rd)    # a tenth of the histories' rule
    if case == ph.MULTI_CASE:
        B, X0 = jh.columns(oracle, b, ph.MULTI_K, ph.MULTI_SEED)
        for j in range(ph.MULTI_K):
            sc = jh.cycle_scale(Ho, B[:, j], X0[:, j])
            xs = cycle(Ho, X0[:, j], B[:, j])
            xd = cycle(Ho, X0[:, j], B[:, j], coarse_solve=jh.dense_coarse_solve)
            res = float(np.linalg.norm(A @ (xd - xs))) / sc
            rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
            print(f"[periodic] {case} column {j}, reference against reference: residual {res:.2e} scale, iterate {rel:.2e}")
            _note("columns: residual", res)
            _note("columns: iterate", rel)
            assert res <= 0.1 * GPU_TOL and rel <= 0.1 * ph.COLUMN_ITERATE_TOL, (case, j, res, rel)


def test_print_the_reference_figures():
    for what in sorted(WORST):
        print(f"[periodic] reference against reference, largest {what}: {WORST[what]:.2e}")


def test_sparse_lu_meets_the_coarse_bound():
    """the periodic systems of tests/test_gpu_coarse_dictionary.py, solved by a float64 sparse LU: ||A x - b|| / ||b||
    is at most a tenth of the 1e-12 those tests hold the device's cyclic reduction to"""
    import scipy.sparse.linalg as spla
    import test_gpu_coarse_dictionary as cd
    worst = 0.0
    for nb, m, P in cd.PERIODIC_SYSTEMS:
        A, b = cd.periodic_system(nb, m, P)
        assert A.shape == (nb * m, nb * m)
        blocks = [A[:m, :m].toarray()] + [A[j * m:(j + 1) * m, (j - 1) * m:(j + 2) * m].toarray() for j in range(1, 2 * P + 2)]
        for j in range(2, P + 1):      # period P, and no shorter one next door
            assert np.array_equal(blocks[j], blocks[j + P]) and not np.array_equal(blocks[j], blocks[j + 1]), (nb, m, P, j)
        x = spla.spsolve(A, b)
        res = float(np.linalg.norm(A @ x - b) / np.linalg.norm(b))
        print(f"[coarse periodic] sparse LU, nb {nb} m {m} P {P}: ||A x - b|| / ||b|| = {res:.2e}")
        worst = max(worst, res)
        assert res <= 1e-13, (nb, m, P, res)
    print(f"[coarse periodic] sparse LU, largest: {worst:.2e}")
