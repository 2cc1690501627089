"""Helpers of the partitioned-cycle tests with element-patch smoothers (test_dist_patch_cpu.py, test_gpu_dist_patch.py):
the model smoothers of patch_schwarz_model.py / patch_gs_model.py as objects the oracle's smooth_once drives, vectorised
over the patches so that a level of 2048 elements sweeps in milliseconds, an oracle-shaped hierarchy that carries them,
and an engine like dist_helpers.NumpyEngine that smooths through oracle.smooth_once(S, A, u, b, alpha, post=...), so
that the multiplicative model gets its sweep direction.  Test helper, not part of the package."""
import threading

import numpy as np
import torch

import aggmg_oracle as o
import patch_gs_model as gm
import patch_schwarz_model as pm
from dist_helpers import NumpyEngine
from agglomerationmultigrid1d_amd import distributed as D

VARIANTS = ("patchGS0", "patchGS", "patchSchwarz0", "patchSchwarz")


class VecPatchGaussSeidel(o.BlockGaussSeidelRB):
    """patch_gs_model.gs_sweep on the level's block-tridiagonal form (smooth_once calls sweep(..., reverse=post))"""

    def __init__(self, T):
        self.T, self.Z = T, gm.patch_inverses(T)
        self.mBlocks, self.mBlockInds = [], pm.patch_lists(T.m, T.ne)

    def sweep(self, A, u, b, alpha=1.0, reverse=False):
        return gm.gs_sweep(self.T, u, b, alpha, reverse, self.Z)


class VecPatchSchwarz(o.HybridSchwarzSmoother):
    """the hybrid sweep of patch_schwarz_model.BlockTridiag.sweep as apply(r, alpha): smooth_once adds it to u"""

    def __init__(self, T):
        self.T, self.Z = T, np.linalg.inv(T.patch_blocks())
        self.mBlocks, self.mBlockInds = [], pm.patch_lists(T.m, T.ne)

    def apply(self, B, alpha=1.0):
        ne, m = self.T.ne, self.T.m
        r = np.asarray(B, dtype=np.float64).reshape(ne, m)
        t = np.zeros((ne, m))
        y = np.einsum("eij,ej->ei", self.Z, np.concatenate([r[:-1], r[1:]], axis=1))
        t[:-1] += y[:, :m]
        t[1:] += y[:, m:]
        t[1:-1] *= 0.5
        return alpha * t.reshape(-1)


class PatchRef:
    """container with the reference's field names for oracle.multigrid_v_cycle / pcg_ldiv: the operators of a
    UniformDgAggHierarchy (whole domain or a rank's element range) with the smoother list `kinds`"""

    def __init__(self, U, kinds):
        n = U.nlevels
        self.mMeshes = [None] * n
        self.mStiffness = [U.stiffness_csc(k) for k in range(n)]
        self.mInterpolation = [U.interpolation_csc(k) for k in range(n - 1)]
        self.mSmoothers = []
        for k in range(n - 1):
            if kinds[k] == "blockJac":
                A = self.mStiffness[k]
                inds = U.descriptor(k).mBlockInds
                blocks = [o.LU(A[np.ix_(inds[:, i] - 1, inds[:, i] - 1)].toarray()) for i in range(inds.shape[1])]
                self.mSmoothers.append(o.BlockJacobi(blocks, inds))
            else:
                T = pm.BlockTridiag(*U.levels[k]['A'])
                self.mSmoothers.append({"patchGS": VecPatchGaussSeidel, "patchSchwarz": VecPatchSchwarz}[kinds[k]](T))


class SmoothOnceEngine(NumpyEngine):
    """NumpyEngine whose sweeps are oracle.smooth_once (post = True on the way up), plus the engine methods
    distributed.pcg calls"""

    def down(self, x0, b, nPre, alpha):
        H = self.H
        n = len(H.mStiffness)
        self.u[0] = x0.numpy().copy()
        self.rhs[0] = b.numpy().copy()
        for k in range(n - 1):
            if k > 0:
                self.u[k] = np.zeros(H.mStiffness[k].shape[1])
            for _ in range(nPre):
                self.u[k] = o.smooth_once(H.mSmoothers[k], H.mStiffness[k], self.u[k], self.rhs[k], alpha)
            self.rhs[k + 1] = o.csc_adjoint_matvec(H.mInterpolation[k], self.rhs[k] - o.csc_matvec(H.mStiffness[k], self.u[k]))

    def up(self, b, x_out, nPost, alpha):
        H = self.H
        for k in range(len(H.mStiffness) - 2, -1, -1):
            self.u[k] = self.u[k] + o.csc_matvec(H.mInterpolation[k], self.u[k + 1])
            for _ in range(nPost):
                self.u[k] = o.smooth_once(H.mSmoothers[k], H.mStiffness[k], self.u[k], self.rhs[k], alpha, post=True)
        x_out.copy_(torch.from_numpy(self.u[0]))

    def owned_dot(self, ranges, x, y):
        xv, yv = x.numpy(), y.numpy()
        return float(sum(np.dot(xv[lo:hi], yv[lo:hi]) for lo, hi in ranges))

    def residual(self, x, b, r):
        r.copy_(torch.from_numpy(b.numpy() - o.csc_matvec(self.H.mStiffness[0], x.numpy())))

    def neg_apply(self, p, q):
        q.copy_(torch.from_numpy(-o.csc_matvec(self.H.mStiffness[0], p.numpy())))

    def pcg_xr(self, ranges, x, r, p, q, a):
        x.add_(p, alpha=a)
        r.add_(q, alpha=a)
        return self.owned_dot(ranges, r, r)

    def pcg_p(self, p, z, beta):
        p.copy_(z + beta * p)

    def assign(self, dst, src):
        dst.copy_(src)


class ThinLayout(D.RankLayout):
    """a RankLayout whose ghost layers are `thinner` units of coarsest width thinner than halo_widths asks (the
    necessity tests); the widths stay nested"""

    def __init__(self, n_fine, ratios, block_sizes, world, rank, nPre, nPost, smoothers, thinner):
        D.RankLayout.__init__(self, n_fine, ratios, block_sizes, world, rank, nPre, nPost, smoothers=smoothers)
        w = self.W[-1] - thinner
        self.W = [w * int(np.prod(ratios[k:])) for k in range(len(ratios))] + [w]
        for k in range(len(self.W)):
            lo, hi = self.own[k]
            self.loc[k] = (max(0, lo - self.W[k]), min(self.ne[k], hi + self.W[k]))


def thread_ranks(world, fn):
    """run fn(rank, comm) on `world` ThreadComm ranks (threads of this process) -> (results by rank, errors)"""
    g = D.ThreadGroup(world)
    out, errs = [None] * world, []

    def one(r):
        try:
            out[r] = fn(r, D.ThreadComm(g, r))
        except BaseException as exc:
            errs.append((r, exc))
            g.barrier.abort()

    ts = [threading.Thread(target=one, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    return out, errs
