"""The multiplicative two-colour element-patch sweep (aggmg_patch_gs_setup, api.ElementPatchGaussSeidel; DESIGN.md
section 20) in NumPy, as the library defines it.  Test helper, not part of the package.

Level of ne >= 2 elements of m rows, A block tridiagonal in that blocking, patches P_e = {e, e + 1}, e = 0 .. ne - 2,
Z_e = inv(A[P_e, P_e]).  One forward sweep of weight w is the half-sweeps c = 0, 1 (a reverse one: c = 1, 0):

    r = b - A u                                      (from the current u)
    u[P_e] += w Z_e r[P_e]    for every patch e = c (mod 2)

The patches of one colour are disjoint; an element none of them covers keeps its value in that half-sweep.

Three forms: patch_gs_sweep(s) on a dense A, gs_sweep(s) vectorised on a patch_schwarz_model.BlockTridiag (any float
dtype: the longdouble runs of the GPU test), and PatchGaussSeidelModel, a smoother the oracle's smooth_once drives."""
import copy

import numpy as np

import patch_schwarz_model as pm


def colours(reverse=False):
    return (1, 0) if reverse else (0, 1)


def patch_gs_sweep(A, m, ne, u, b, w, reverse=False):
    """one sweep on a dense (or scipy) A by the definition above, in float64"""
    A = pm.dense(A)
    u = np.array(u, dtype=np.float64)
    for c in colours(reverse):
        r = b - A @ u
        for e in range(c, ne - 1, 2):
            idx = np.arange(e * m, (e + 2) * m)
            u[idx] += w * np.linalg.solve(A[np.ix_(idx, idx)], r[idx])
    return u


def patch_gs_sweeps(A, m, ne, u, b, weights, reverse=False):
    for w in weights:
        u = patch_gs_sweep(A, m, ne, u, b, w, reverse)
    return u


def _matvec(T, U, dtype):
    """T's blocks times U (ne, m), in dtype"""
    d, lo, hi = (np.asarray(x, dtype=dtype) for x in (T.diag, T.sub, T.sup))
    Y = np.einsum("eij,ej->ei", d, U)
    Y[1:] += np.einsum("eij,ej->ei", lo[1:], U[:-1])
    Y[:-1] += np.einsum("eij,ej->ei", hi[:-1], U[1:])
    return Y


def patch_inverses(T, dtype=np.float64):
    """(ne - 1, 2m, 2m): Z_e of the BlockTridiag T; in a wider dtype than float64 by two steps of Newton's iteration
    X <- X (2 I - B X) on the float64 inverse (quadratic: 1e-16 -> 1e-32, below any longdouble's precision)"""
    B = T.patch_blocks()
    X = np.linalg.inv(B)
    if np.dtype(dtype) == np.float64:
        return X
    B, X = B.astype(dtype), X.astype(dtype)
    eye2 = 2 * np.eye(B.shape[1], dtype=dtype)[None]
    for _ in range(2):
        X = np.einsum("eij,ejk->eik", X, eye2 - np.einsum("eij,ejk->eik", B, X))
    return X


def gs_sweep(T, u, b, w, reverse=False, zinv=None, dtype=np.float64):
    """one sweep on a BlockTridiag, vectorised over the patches of a colour"""
    ne, m = T.ne, T.m
    Z = patch_inverses(T, dtype) if zinv is None else zinv
    U = np.array(u, dtype=dtype).reshape(ne, m)
    Bv = np.asarray(b, dtype=dtype).reshape(ne, m)
    w = np.asarray(w, dtype=dtype)
    for c in colours(reverse):
        R = Bv - _matvec(T, U, dtype)
        es = np.arange(c, ne - 1, 2)
        if len(es):
            y = np.einsum("eij,ej->ei", Z[es], np.concatenate([R[es], R[es + 1]], axis=1))
            U[es] += w * y[:, :m]
            U[es + 1] += w * y[:, m:]
    return U.reshape(-1)


def gs_sweeps(T, u, b, weights, reverse=False, dtype=np.float64):
    Z = patch_inverses(T, dtype)
    u = np.asarray(u, dtype=dtype)
    for w in weights:
        u = gs_sweep(T, u, b, w, reverse, Z, dtype)
    return u


def make_model_smoother(o, A, m, ne, weight=None):
    """the multiplicative patch smoother as an object of the oracle: a subclass of its BlockGaussSeidelRB, so that
    smooth_once calls sweep(A, u, b, alpha, reverse=post).  weight: used in place of the cycle's alpha (the rows
    "weight 1 on level 0" of DESIGN.md section 20); None: the cycle's alpha."""
    Ad = pm.dense(A)
    inds = pm.patch_lists(m, ne)

    class PatchGaussSeidelModel(o.BlockGaussSeidelRB):
        def sweep(self, A_, u, b, alpha=1.0, reverse=False):
            u = np.array(u, dtype=np.float64)
            w = alpha if self.weight is None else self.weight
            for c in colours(reverse):
                r = b - o.csc_matvec(A_, u)
                for e in range(c, len(self.mBlocks), 2):
                    idx = self.mBlockInds[:, e] - 1
                    u[idx] += w * self.mBlocks[e].solve(r[idx])
            return u

    S = PatchGaussSeidelModel([o.LU(Ad[np.ix_(col - 1, col - 1)]) for col in inds.T], inds)
    S.weight = weight
    return S


def with_gs_smoothers(o, H, levels, weights=None):
    """a copy of the oracle hierarchy H with the multiplicative patch smoother on `levels`; weights: {level: weight}
    overriding the cycle's alpha there"""
    H2 = copy.copy(H)
    H2.mSmoothers = list(H.mSmoothers)
    for k in levels:
        m, ne = pm.level_shape(H, k)
        H2.mSmoothers[k] = make_model_smoother(o, H.mStiffness[k], m, ne, (weights or {}).get(k))
    return H2


def cycles_to_tol(o, H, b, nPre, nPost, alpha=2.0 / 3.0, tol=1e-8, maxiter=200):
    return pm.cycles_to_tol(o, H, b, nPre, nPost, alpha, tol, maxiter)


def pcg_its(o, H, b, nPre, nPost, alpha=2.0 / 3.0, tol=1e-8, maxiter=100):
    """(iterations of the oracle's pcg_ldiv from the zero guess, true relative residual of its result)"""
    x, it, _ = o.pcg_ldiv(H, b, None, maxiter, tol, nPre, nPost, alpha)
    A = H.mStiffness[0]
    return it, np.linalg.norm(o.csc_matvec(A, x) - b) / np.linalg.norm(b)


def cycle_asymmetry(o, H, n, alpha=2.0 / 3.0, seeds=(1, 2), N=None):
    """|<M r1, r2> - <r1, M r2>| / |<M r1, r2>| of the V(n, n) cycle M from the zero guess"""
    N = H.mStiffness[0].shape[0] if N is None else N
    r1, r2 = o.splitmix_normal(N, seeds[0]), o.splitmix_normal(N, seeds[1])
    z = np.zeros(N)
    a = float(o.multigrid_v_cycle(H, z, r1, n, n, alpha) @ r2)
    c = float(r1 @ o.multigrid_v_cycle(H, z, r2, n, n, alpha))
    return abs(a - c) / abs(a)
