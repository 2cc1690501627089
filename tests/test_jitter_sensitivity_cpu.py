"""Why the uniform-ratio fused kernels are tested on jittered meshes (tests/test_gpu_jittered_uniform_ratio.py), shown
with the oracle alone: one index error at one interior element of one level -- the right-hand neighbour's inverse block,
transfer block or operator block row in place of the element's own (tests/jitter_helpers.py) -- and the change of one
V(3,3) from a random first iterate, ||A (x_mut - x)|| in units of scale = ||b|| + ||A x0||.

 * On the jittered mesh every such error moves the cycle by at least 1e-10 scale, 100 times the 1e-12 scale the GPU
   tests allow (measured: 2.8e-8 at the least -- the smoother error on level 3 of b2 -- and up to 1.0e-2).
 * On the uniform mesh of the same shape none moves it by 1e-12 scale (measured: exactly 0 at n = 2048 and 1024, at
   most 9.7e-17 at n = 768 and 1536), so no comparison on a uniform mesh can see them.

With pAgg = 0 the transfer is piecewise constant: its blocks do not depend on the elements' positions, every
agglomerate's block is the same on any mesh, and the transfer error is no error.  It is asserted to be exactly 0 there.

The last test holds the reference against itself (sparse against dense LU at the coarsest level) on the jittered meshes
at every sweep count the GPU tests use, to show that their bounds are the reference's to give."""
import numpy as np
import pytest

import jitter_helpers as jh

GPU_TOL = jh.RESIDUAL_TOL   # tests/test_gpu_jittered_uniform_ratio.py: ||A (x - x_ref)|| <= GPU_TOL * scale
SEED = jh.X0_SEED


@pytest.fixture(scope="module")
def built(oracle):
    cache = {}

    def get(case, jitter):
        if (case, jitter) not in cache:
            cache[case, jitter] = jh.build(oracle, case, jitter)
        return cache[case, jitter]
    return get


def _changes(oracle, Ho, b):
    """{(level, mutation): ||A (x_mut - x)|| / scale} of one V(3,3); the hierarchy is checked to be itself again"""
    x0 = oracle.splitmix_normal(len(b), SEED)
    A = Ho.mStiffness[0]
    scale = jh.cycle_scale(Ho, b, x0)
    x = oracle.multigrid_v_cycle(Ho, x0, b)
    out = {}
    for k in jh.smoothed_levels(Ho):
        for name, mutate in jh.MUTATIONS.items():
            with mutate(Ho, k):
                xm = oracle.multigrid_v_cycle(Ho, x0, b)
            out[k, name] = float(np.linalg.norm(A @ (xm - x))) / scale
    assert np.array_equal(oracle.multigrid_v_cycle(Ho, x0, b), x), "a mutation was not undone"
    return out


@pytest.mark.parametrize("case", list(jh.CASES))
def test_index_errors_show_on_the_jittered_mesh_only(oracle, built, case):
    pAgg = jh.CASES[case][2]
    moved = {jitter: _changes(oracle, *built(case, jitter)) for jitter in (True, False)}
    levels = sorted({k for k, _ in moved[True]})
    assert levels == list(range(jh.CASES[case][3])) and moved[True].keys() == moved[False].keys()
    print(f"\n[jitter sensitivity] {case} {jh.CASES[case]}: change of V(3,3) / scale, jittered | uniform")
    for k in levels:
        print(f"  level {k}: " + "   ".join(f"{name} {moved[True][k, name]:.2e} | {moved[False][k, name]:.2e}" for name in jh.MUTATIONS))
    for (k, name), v in moved[True].items():
        if name == "transfer" and pAgg == 0:
            # one constant per agglomerate: the block is the same for every agglomerate of every mesh
            assert v == 0.0 and moved[False][k, name] == 0.0, (case, k, v)
            continue
        assert v >= 100.0 * GPU_TOL, (case, k, name, v)
        assert moved[False][k, name] < GPU_TOL, (case, k, name, moved[False][k, name])


SWEEPS = {"c34": ((3, 3), (1, 2), (0, 3), (8, 8))}


@pytest.mark.parametrize("case", list(jh.CASES))
def test_reference_against_reference(oracle, built, case):
    """measured on the jittered meshes, one cycle from the GPU tests' first iterate: ||A (x_dense - x_sparse)|| / scale
    4.3e-17 .. 5.3e-16 at V(3,3) and 3.6e-15 at most at c34's other sweep counts; ||x_dense - x_sparse|| / ||x|| at most
    2.1e-11.  Loops from zero: residual at most 4.7e-15 ||b||; iterate at most 2.4e-11 after the first cycle and up to
    3.6e-10 after later ones (jitter_helpers.loop_iterate_tol); ||A x_k - b|| equal to 6e-13 relative.  The K-column
    tests' columns: residual at most 6.8e-15, iterate at most 1.5e-11.  The residual figures are asserted below a tenth
    of the GPU tests' 1e-12, the iterate figures below the bounds the GPU tests use"""
    Ho, b = built(case, True)
    x0 = oracle.splitmix_normal(len(b), SEED)
    A = Ho.mStiffness[0]
    scale = jh.cycle_scale(Ho, b, x0)
    for nPre, nPost in SWEEPS.get(case, ((3, 3),)):
        xs = oracle.multigrid_v_cycle(Ho, x0, b, nPre=nPre, nPost=nPost, alpha=jh.ALPHA)
        xd = oracle.multigrid_v_cycle(Ho, x0, b, nPre=nPre, nPost=nPost, alpha=jh.ALPHA, coarse_solve=jh.dense_coarse_solve)
        res = float(np.linalg.norm(A @ (xd - xs))) / scale
        rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
        print(f"[jitter sensitivity] {case} V({nPre},{nPost}) reference against reference: residual {res:.2e} scale, iterate {rel:.2e}")
        assert res <= 0.1 * GPU_TOL and rel <= jh.ITERATE_TOL, (case, nPre, nPost, res, rel)
    # the loops' rule: V(3,3) repeated from a zero first iterate, every iterate by the same two bounds with scale = ||b||
    xs = xd = np.zeros(len(b))
    nb = float(np.linalg.norm(b))
    for cyc in range(1, jh.NCYC + 1):
        xs = oracle.multigrid_v_cycle(Ho, xs, b)
        xd = oracle.multigrid_v_cycle(Ho, xd, b, coarse_solve=jh.dense_coarse_solve)
        res = float(np.linalg.norm(A @ (xd - xs))) / nb
        rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
        rs, rd = float(np.linalg.norm(A @ xs - b)), float(np.linalg.norm(A @ xd - b))
        print(f"[jitter sensitivity] {case} cycle {cyc} from zero, reference against reference: residual {res:.2e} ||b||, "
              f"iterate {rel:.2e}, ||A x - b|| {rs:.6e} / {rd:.6e}")
        assert res <= 0.1 * GPU_TOL and rel <= jh.loop_iterate_tol(cyc), (case, cyc, res, rel)
        assert np.isclose(rd, rs, rtol=1e-9, atol=1e-12 * nb), (case, cyc, rs, rd)    # a tenth of the histories' rule
    # the K-column tests' inputs
    if case in jh.MULTI_CASES:
        B, X0 = jh.columns(oracle, b, 8, jh.MULTI_SEED)
        for j in range(8):
            scale = jh.cycle_scale(Ho, B[:, j], X0[:, j])
            xs = oracle.multigrid_v_cycle(Ho, X0[:, j], B[:, j])
            xd = oracle.multigrid_v_cycle(Ho, X0[:, j], B[:, j], coarse_solve=jh.dense_coarse_solve)
            res = float(np.linalg.norm(A @ (xd - xs))) / scale
            rel = float(np.linalg.norm(xd - xs) / np.linalg.norm(xs))
            print(f"[jitter sensitivity] {case} column {j} reference against reference: residual {res:.2e} scale, iterate {rel:.2e}")
            assert res <= 0.1 * GPU_TOL and rel <= jh.ITERATE_TOL, (case, j, res, rel)
