"""distributed.fgmres on the CPU: flexible GMRES around the element-partitioned V-cycle, ranks as threads over ThreadComm,
NumPy engines (oracle arithmetic, the model patch smoothers of dist_patch_helpers) in place of the GPU kernels, against
fgmres_model (the oracle's cycle on the whole domain); the package's host least-squares object against the model's; the
rank-ordered vector sum of the communicators.

Tolerance on the residual history.  The partitioned loop differs from the model only in the order of its sums: a global
dot product is the rank-ordered sum of the ranks' owned terms.  How far that moves the history is measured reference
against reference: `pieces_fgmres` is the model's recurrence with every dot product and norm summed in k rank-sized
pieces, added in rank order.  The movement depends on k irregularly (the histories below move by 1e-12 for some piece
counts and by 1e-9 for others), so ALL of k = 1 .. 8 are run; the figure of a shape is the largest relative movement of
any of the first 8 entries against fgmres_model's own history, and the bound on a partitioned run is ten times the figure
(the margin over one host's measurement, as in test_distributed_pcg_cpu: the BLAS order inside a piece, the GPU's
summation trees).  Measured where this file was written:

    shape                                                        entries   worst movement   bound
    "schwarz0_v33"      patchSchwarz0, n = 2048, V(3,3), restart 30    6      6.80e-10      6.80e-9
    "schwarz0_v33_r3"   the same, restart 3 (cut at 8 entries)         8      1.22e-8       1.22e-7
    "schwarz_v21"       patchSchwarz, n = 2048, V(2,1), restart 30     8      1.22e-9       1.22e-8
    "config5_v21"       CG p = 4 > 2 > 1 > DG p = 0, n = 2^14, V(2,1)  6      1.53e-11      1.53e-10

test_split_reference_stays_within_the_bound repeats the measurement wherever the suite runs, prints it and holds it to
the bound.  The config-5 figure is measured at the size the GPU test uses it at (at n = 2048 it is 4.1e-12).

Stopping tolerances are the geometric mean of two consecutive entries of the reference history whose ratio is at least 3
(asserted): a movement within the bound cannot change the count."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")) if p not in sys.path]

import aggmg_oracle as o                                                   # noqa: E402
import dist_patch_helpers as dh                                            # noqa: E402
from fgmres_model import Givens, fgmres_model                              # noqa: E402
from agglomerationmultigrid1d_amd import distributed as D                  # noqa: E402
from agglomerationmultigrid1d_amd.uniform import UniformDgAggHierarchy     # noqa: E402

N, P, RATIOS, ALPHA = 2048, 3, (4, 2, 2), 2.0 / 3.0
M = [P + 1] + [2] * len(RATIOS)
EPS = np.finfo(np.float64).eps

# name -> what is run: the smoother spelling (None: config 5's CG chain), the size, the sweeps, the restart length and
# the number of history entries compared
SHAPES = {
    "schwarz0_v33": dict(smoother="patchSchwarz0", n=N, nPre=3, nPost=3, restart=30, entries=6),
    "schwarz0_v33_r3": dict(smoother="patchSchwarz0", n=N, nPre=3, nPost=3, restart=3, entries=8),
    "schwarz_v21": dict(smoother="patchSchwarz", n=N, nPre=2, nPost=1, restart=30, entries=8),
    "config5_v21": dict(smoother=None, n=2**14, nPre=2, nPost=1, restart=30, entries=6),
}
HIST_DRIFT_MEASURED = {"schwarz0_v33": 6.80e-10, "schwarz0_v33_r3": 1.22e-8, "schwarz_v21": 1.22e-9,
                       "config5_v21": 1.53e-11}      # reference against reference over k = 1 .. 8, see above


def hist_rtol(shape):
    return 10 * HIST_DRIFT_MEASURED[shape]


def stop_tolerance(hist, count, nb):
    """the relative tolerance met after exactly `count` iterations: the geometric mean of the last entry that misses it
    and the first that meets it (hist[count - 2], hist[count - 1]), which must be at least a factor 3 apart"""
    assert count >= 2 and hist[count - 2] >= 3 * hist[count - 1], (count, hist)
    return math.sqrt(hist[count - 2] * hist[count - 1]) / nb


class FgmresNumpyEngine(dh.SmoothOnceEngine):
    """SmoothOnceEngine + the engine methods distributed.fgmres calls beyond pcg's, in NumPy"""

    def new_basis(self, nvec, n):
        return torch.zeros((int(nvec), int(n) + (int(n) & 1)), dtype=torch.float64)

    def owned_multi_dot(self, ranges, V, nvec, w):
        return np.array([self.owned_dot(ranges, w, V[i][:w.numel()]) for i in range(nvec)])

    def owned_multi_axpy_norm(self, ranges, V, nvec, coef, w, sumsq=True):
        wv = w.numpy()
        for i in range(nvec):
            wv += float(coef[i]) * V[i][:w.numel()].numpy()
        return self.owned_dot(ranges, w, w) if sumsq else None

    def div_scalar(self, w, s, v):
        v.copy_(w / s)


def pieces_fgmres(H, b, k, restart, maxiter, tol, nPre, nPost):
    """fgmres_model's recurrence (classical Gram-Schmidt) with every dot product and norm summed in k rank-sized
    pieces, added in rank order"""
    A = H.mStiffness[0]
    n = A.shape[0]
    cut = [n * r // k for r in range(k + 1)]

    def dot(u, v):
        acc = float(u[cut[0]:cut[1]] @ v[cut[0]:cut[1]])
        for r in range(1, k):
            acc = acc + float(u[cut[r]:cut[r + 1]] @ v[cut[r]:cut[r + 1]])
        return acc

    x, zero = np.zeros(n), np.zeros(n)
    nb = np.sqrt(dot(b, b))
    res, done = [], False
    while not done and len(res) < maxiter:
        r = b - o.csc_matvec(A, x)
        beta = np.sqrt(dot(r, r))
        if beta == 0.0 or beta < tol * nb or not np.isfinite(beta):
            break
        m = min(restart, maxiter - len(res))
        V, Z = np.zeros((m + 1, n)), np.zeros((m, n))
        V[0] = r / beta
        ls = Givens(beta, m)
        finite = True
        for j in range(m):
            Z[j] = o.multigrid_v_cycle(H, zero, V[j], nPre, nPost, ALPHA)
            w = o.csc_matvec(A, Z[j])
            h = np.array([dot(V[i], w) for i in range(j + 1)])
            for i in range(j + 1):
                w = w - h[i] * V[i]
            hn = np.sqrt(dot(w, w))
            rj = ls.push(np.concatenate([h, [hn]]))
            res.append(float(rj))
            if not np.isfinite(rj):
                finite, done = False, True
                break
            if rj < tol * nb or hn == 0.0:
                done = True
                break
            if j + 1 < m:
                V[j + 1] = w / hn
        if not finite:
            break
        x = x + Z[:ls.k].T @ ls.solve()
    return x, len(res), res


_refs = {}


def reference(shape):
    """the whole-domain hierarchy of a shape and fgmres_model's history on it (two entries more than are compared),
    computed once and left unchanged"""
    if shape not in _refs:
        s = SHAPES[shape]
        if s["smoother"] is None:
            Hg, bg = o.build_cg_hierarchy(s["n"], ps=(4, 2, 1), nDG=1, pDG=0)
            bg, Ug = np.array(bg, dtype=np.float64), None
        else:
            Ug = UniformDgAggHierarchy(s["n"], p=P, pAgg=1, ratios=RATIOS)
            Hg = dh.PatchRef(Ug, D.smoother_kinds(s["smoother"], len(RATIOS)))
            bg = np.array(Ug.rhs())
        _, _, hist = fgmres_model(o, Hg, bg, restart=s["restart"], maxiter=s["entries"] + 2, tol=1e-30, nPre=s["nPre"],
                                  nPost=s["nPost"], alpha=ALPHA)
        bg.setflags(write=False)
        _refs[shape] = dict(Ug=Ug, Hg=Hg, bg=bg, nb=float(np.linalg.norm(bg)), hist=[float(v) for v in hist])
    return _refs[shape]


# ---- 1. the host least-squares object ---------------------------------------------------------------------------------------
def test_host_gmres_is_the_model_givens_bit_for_bit():
    """D.HostGmres (csrc/host_gmres.hpp restated in the package) against fgmres_model.Givens on random Hessenberg columns,
    a zero column among them: every returned residual norm, every rotation, g and the rotated columns bit for bit.  The
    back-substitution is compared on the nonsingular run only and to rounding, not bit for bit: the header (and the
    package) subtract the products one at a time, the model takes a dot product of the row -- per entry at most
    (k + 2) eps sum |R_il y_l| / |R_ii| apart (k products, one division)."""
    rng = np.random.default_rng(17)
    for m, zero_col in ((1, None), (7, None), (30, None), (9, 4), (64, None)):
        beta = float(abs(rng.standard_normal()) + 0.5)
        mine, model = D.HostGmres(), Givens(beta, m)
        mine.start(beta)
        for j in range(m):
            h = rng.standard_normal(j + 2)
            h[j + 1] = abs(h[j + 1])
            if j == zero_col:
                h[:] = 0.0
            assert mine.push(h) == model.push(h)
            assert mine.size() == model.k == j + 1
            assert mine.c[:j + 1] == model.c[:j + 1].tolist() and mine.s[:j + 1] == model.s[:j + 1].tolist()
            assert mine.g[:j + 2] == model.g[:j + 2].tolist()
            assert mine.r[j][:j + 2] == model.R[:j + 2, j].tolist()
        if zero_col is None:
            y, ym = np.array(mine.solve()), model.solve()
            R = np.triu(model.R[:m, :m])
            bound = (m + 2) * EPS * (np.abs(R) @ np.abs(ym) + np.abs(model.g[:m])) / np.abs(np.diag(R))
            # (entry i also inherits the differences of the entries behind it: solve the triangular system for them)
            assert np.all(np.abs(y - ym) <= _propagated(R, bound))
        else:
            assert not np.all(np.isfinite(mine.solve()))          # the division by the zero pivot, as in C++: no exception
    with pytest.raises(IndexError):
        full = D.HostGmres()
        full.start(1.0)
        for j in range(D.FGMRES_MAX_RESTART + 1):
            full.push(np.ones(j + 2))


def _propagated(R, bound):
    """|dy| <= bound + |R_ii|^-1 sum_{l > i} |R_il| |dy_l|, solved from the last entry up"""
    m = len(bound)
    dy = np.zeros(m)
    for i in range(m - 1, -1, -1):
        dy[i] = bound[i] + (np.abs(R[i, i + 1:]) @ dy[i + 1:]) / abs(R[i, i])
    return dy


# ---- 2. the rank-ordered vector sum ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 8])
def test_sum_vec_adds_in_rank_order(world):
    """identical bits on every rank, equal to the explicit rank-order loop over the ranks' vectors, and a vector of one
    entry agrees with Comm.sum.

    The last property as the specification words it, sum_vec([v])[0] == sum(v) bit for bit, holds on 2 ranks (and up to
    7): there sum()'s np.sum IS the rank-order chain.  On 8 ranks NumPy adds the eight terms as a tree, ((a0 + a1) + (a2 +
    a3)) + ((a4 + a5) + (a6 + a7)) in its 8-lane form, so the chain sum_vec is REQUIRED to be and sum() differ in the last
    bit on about half of all random inputs (measured: 982 of 2000) -- the two requirements exclude each other there, and
    sum() is not to be changed.  On 8 ranks the test therefore asks for the bit-for-bit agreement on terms whose sums are
    exact in any order (multiples of 2^-20 below 2^20), and on general terms for agreement within the reordering bound
    7 eps sum |a_r| (seven additions, one rounding each)."""
    rng = np.random.default_rng(23)
    general = rng.standard_normal((world, 9)) * 10.0 ** rng.integers(-3, 4, (world, 9))
    exact = rng.integers(-2**40, 2**40, (world, 1)).astype(np.float64) * 2.0**-20

    def rank_fn(rank, comm):
        return (comm.sum_vec(general[rank]), comm.sum_vec([general[rank][0]]), comm.sum(general[rank][0]),
                comm.sum_vec(exact[rank]), comm.sum(exact[rank][0]), comm.sum_vec(list(general[rank][:3])))

    out, errs = dh.thread_ranks(world, rank_fn)
    assert not errs, errs
    want = general[0].copy()
    for r in range(1, world):
        want = want + general[r]
    for vec, one, s, ex, exs, lst in out:
        assert isinstance(vec, np.ndarray) and vec.dtype == np.float64 and vec.shape == (9,)
        assert vec.tobytes() == want.tobytes() == out[0][0].tobytes()
        assert one.shape == (1,) and one[0] == want[0] and np.array_equal(lst, want[:3])
        assert ex[0] == exs
        if world < 8:
            assert one[0] == s
        else:
            assert abs(one[0] - s) <= (world - 1) * EPS * float(np.sum(np.abs(general[:, 0])))


def test_sum_vec_on_one_rank_is_a_copy():
    class One(D.Comm):
        def __init__(self):
            self.world, self.rank, self.staged = 1, 0, True

    v = np.array([1.5, -2.25, 1e-300])
    got = One().sum_vec(v)
    assert np.array_equal(got, v) and got is not v


# ---- 3. the measurement behind the history bounds --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_split_reference_stays_within_the_bound(shape):
    """the model against itself with its sums in k = 1 .. 8 pieces: the first `entries` entries move by at most ten
    times the recorded figure (the figure itself is printed)"""
    s, ref = SHAPES[shape], reference(shape)
    hist = np.array(ref["hist"][:s["entries"]])
    assert all(hist[i] >= 3 * hist[i + 1] for i in range(len(hist) - 1)), hist       # (3.4 .. 62 when this was written)
    worst = 0.0
    for k in range(1, 9):
        _, it, res = pieces_fgmres(ref["Hg"], np.array(ref["bg"]), k, s["restart"], s["entries"], 1e-30, s["nPre"], s["nPost"])
        assert it == s["entries"]
        move = float(np.max(np.abs(np.array(res) - hist) / hist))
        print(f"{shape}, {k} pieces: the history moves by {move:.3e}")
        worst = max(worst, move)
    print(f"{shape}: worst movement {worst:.3e} (recorded {HIST_DRIFT_MEASURED[shape]:.2e}, bound {hist_rtol(shape):.2e})")
    assert worst <= hist_rtol(shape)


# ---- 4. the partitioned loop against the model -----------------------------------------------------------------------------
def make_rank(shape, world, rank, comm, nPre=None, nPost=None):
    s, ref = SHAPES[shape], reference(shape)
    kinds = D.smoother_kinds(s["smoother"], len(RATIOS))
    layout = D.RankLayout(s["n"], RATIOS, M, world, rank, s["nPre"] if nPre is None else nPre,
                          s["nPost"] if nPost is None else nPost, smoothers=kinds)
    U = UniformDgAggHierarchy(s["n"], p=P, pAgg=1, ratios=RATIOS, elem_range=layout.loc[0])
    Ac = ref["Ug"].stiffness_csc(ref["Ug"].nlevels - 1)
    dv = D.DistributedVCycle(FgmresNumpyEngine(o, dh.PatchRef(U, kinds), Ac), layout, comm)
    return dv, layout, torch.from_numpy(U.rhs().copy())


def true_residual(ref, parts):
    """||b - A x|| of the iterate gathered from the ranks' owned parts ((lo, hi) in elements, values)"""
    xg = np.empty(len(ref["bg"]))
    for (lo, hi), xown in parts:
        xg[lo * (P + 1):hi * (P + 1)] = xown
    A = ref["Hg"].mStiffness[0]
    return float(np.linalg.norm(ref["bg"] - o.csc_matvec(A, xg))), xg


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("shape", ["schwarz0_v33", "schwarz0_v33_r3", "schwarz_v21"])
def test_partitioned_fgmres_matches_the_model(shape, world):
    """(a) hybrid patchSchwarz0 V(3,3), restart 30; (b) the same with restart 3, cut at 8 entries -- two full restart
    cycles and a third begun; (c) hybrid patchSchwarz on every level, V(2,1), which pcg refuses.  On 2 and 4 thread
    ranks: the model's count on every rank, one history on all ranks bit for bit, within the bound of the shape; and the
    gathered owned iterate's true residual agrees with the last entry as closely as the model's own does (ten times the
    model's gap, plus the rounding of forming b - A x: 10 eps || |b| + |A| |x| ||)."""
    s, ref = SHAPES[shape], reference(shape)
    cut = s["restart"] < s["entries"]
    tol = 1e-30 if cut else stop_tolerance(ref["hist"], s["entries"], ref["nb"])
    maxiter = s["entries"] if cut else 50
    kw = dict(restart=s["restart"], maxiter=maxiter, tol=tol, nPre=s["nPre"], nPost=s["nPost"], alpha=ALPHA)
    xo, ito, reso = fgmres_model(o, ref["Hg"], np.array(ref["bg"]), **kw)
    assert ito == s["entries"] and reso == ref["hist"][:ito]
    A = ref["Hg"].mStiffness[0]
    gap_o = abs(float(np.linalg.norm(ref["bg"] - o.csc_matvec(A, xo))) - reso[-1])
    floor = 10 * EPS * float(np.linalg.norm(np.abs(ref["bg"]) + o.csc_matvec(abs(A), np.abs(xo))))

    def rank_fn(rank, comm):
        dv, layout, b = make_rank(shape, world, rank, comm)
        x, it, res = D.fgmres(dv, b, **kw)
        return it, res, (layout.own[0], x.numpy()[layout.owned_slice(0)].copy())

    out, errs = dh.thread_ranks(world, rank_fn)
    assert not errs, errs
    true, xg = true_residual(ref, [part for _, _, part in out])
    for it, res, _ in out:
        rel = float(np.max(np.abs(np.array(res) - np.array(reso)) / np.array(reso)))
        assert it == ito == len(res)
        assert res == out[0][1]                    # bit for bit across ranks
        assert rel <= hist_rtol(shape), rel
    print(f"{shape} on {world} ranks: {ito} iterations, history within {rel:.3e} of the model's (bound {hist_rtol(shape):.2e}); "
          f"last entry {out[0][1][-1]:.6e}, true residual {true:.6e} (model's gap {gap_o:.3e}, floor {floor:.3e})")
    assert abs(true - out[0][1][-1]) <= 10 * gap_o + floor
    assert np.max(np.abs(xg - xo)) <= 1e-6 * np.max(np.abs(xo))


# ---- 5. arguments, start vectors ---------------------------------------------------------------------------------------------
def test_argument_handling_and_nonzero_start():
    """restart outside 1 .. 64 and sweep counts above the layout's halo widths raise ValueError before any rank
    communicates (the other rank would wait for ever otherwise: the ranks are joined under a time limit); nPre != nPost is
    accepted; maxiter = 0 returns the start vector (zeros without one), 0 and []; a nonzero x0 whose ghosts are wrong is
    left alone and converges to the solution of the same system: the gathered iterate's true residual meets the last
    entry with the margin of the test above."""
    shape, world, tol = "schwarz0_v33", 2, 1e-9
    ref = reference(shape)
    x0g = o.splitmix_normal(N * (P + 1), 11)

    def rank_fn(rank, comm):
        dv, layout, b = make_rank(shape, world, rank, comm)
        for bad in (0, -1, 65):
            with pytest.raises(ValueError, match="restart"):
                D.fgmres(dv, b, restart=bad)
        with pytest.raises(ValueError, match="halo"):
            D.fgmres(dv, b, nPre=4, nPost=3)
        with pytest.raises(ValueError, match="halo"):
            D.fgmres(dv, b, nPre=3, nPost=4)
        lo, hi = layout.loc[0]
        sl = layout.owned_slice(0)
        bad = torch.from_numpy(x0g[lo * (P + 1):hi * (P + 1)].copy())
        bad[:sl.start] = 5.0
        bad[sl.stop:] = -7.0
        keep = bad.clone()
        xs, its, ress = D.fgmres(dv, b, x0=bad, maxiter=0)
        assert its == 0 and ress == [] and torch.equal(xs, bad) and xs is not bad
        xz, itz, resz = D.fgmres(dv, b, maxiter=0)
        assert itz == 0 and resz == [] and xz.numel() == bad.numel() and not xz.any()
        x, it, res = D.fgmres(dv, b, x0=bad, restart=5, maxiter=60, tol=tol, nPre=3, nPost=2)
        assert torch.equal(bad, keep)                       # the caller's vector is left alone
        # a start vector that already solves the system to the tolerance: no iteration, x is that vector
        xe, ite, rese = D.fgmres(dv, b, x0=x, maxiter=60, tol=2 * tol, nPre=3, nPost=2)
        assert ite == 0 and rese == [] and torch.equal(xe[sl], x[sl])
        return it, res, (layout.own[0], x.numpy()[sl].copy())

    out, errs = dh.thread_ranks(world, rank_fn)
    assert not errs, errs
    true, xg = true_residual(ref, [part for _, _, part in out])
    A = ref["Hg"].mStiffness[0]
    floor = 10 * EPS * float(np.linalg.norm(np.abs(ref["bg"]) + o.csc_matvec(abs(A), np.abs(xg))))
    for it, res, _ in out:
        assert it == len(res) < 60 and res == out[0][1] and res[-1] < tol * ref["nb"]
    print(f"nonzero x0, V(3,2), restart 5: {out[0][0]} iterations, last entry {out[0][1][-1]:.6e}, true residual {true:.6e}")
    # (the model's own gap on this shape is printed by the test above: 1e-12 relative; 1 % is far outside it and far
    # inside what a wrong iterate would show)
    assert abs(true - out[0][1][-1]) <= 0.01 * out[0][1][-1] + floor
