"""The element-patch Schwarz sweep (aggmg_patch_schwarz_setup) in NumPy, as the library defines it,
and the helpers that put the oracle's HybridSchwarzSmoother on the same lists.  Test helper, not part of the package.

Level of ne elements of m rows, A block tridiagonal in that blocking.  Patches P_e = {e, e + 1}, e = 0 .. ne - 2 (one
patch {0} for ne = 1), Z_e = inv(A[P_e, P_e]), c_e = patches covering element e.  One sweep with weight w:

    r = b - A u
    t[row i of element e] = (Z_{e-1} r[P_{e-1}])[m + i] + (Z_e r[P_e])[i]      (a patch that does not exist adds nothing)
    u += w (t / c_e)   (hybrid)        u += w t   (additive)
"""
import copy

import numpy as np


def patch_lists(m, ne, width=2):
    """(w m) x nb index lists, 1-based, column e = rows of the elements e .. e + w - 1, w = min(width, ne)"""
    w = min(width, ne)
    nb = ne - w + 1
    return np.arange(nb, dtype=np.int64)[None, :] * m + np.arange(1, w * m + 1, dtype=np.int64)[:, None]


def patch_counts(m, ne, width=2):
    """per row, the number of patches covering it"""
    c = np.zeros(m * ne)
    for col in patch_lists(m, ne, width).T:
        c[col - 1] += 1.0
    return c


def dense(A):
    return A.toarray() if hasattr(A, "toarray") else np.asarray(A, dtype=np.float64)


def patch_sweep(A, m, ne, u, b, w, hybrid=True):
    """one sweep by the definition above, in float64"""
    A = dense(A)
    u = np.asarray(u, dtype=np.float64)
    r = b - A @ u
    t = np.zeros(m * ne)
    if ne == 1:
        t += np.linalg.solve(A, r)
    for e in range(ne - 1):
        idx = np.arange(e * m, (e + 2) * m)
        t[idx] += np.linalg.solve(A[np.ix_(idx, idx)], r[idx])
    if hybrid:
        t = t / patch_counts(m, ne)
    return u + w * t


def patch_sweeps(A, m, ne, u, b, weights, hybrid=True):
    for w in weights:
        u = patch_sweep(A, m, ne, u, b, w, hybrid)
    return u


def oracle_patch_smoother(o, A, m, ne, width=2, hybrid=True):
    """the oracle's HybridSchwarzSmoother (AdditiveSchwarzSmoother) on the element-patch lists"""
    Ad = dense(A)
    inds = patch_lists(m, ne, width)
    blocks = [o.LU(Ad[np.ix_(col - 1, col - 1)]) for col in inds.T]
    if hybrid:
        return o.HybridSchwarzSmoother(blocks, inds, patch_counts(m, ne, width))
    return o.AdditiveSchwarzSmoother(blocks, inds)


def level_shape(H, k):
    """(rows per element, elements) of level k of an oracle hierarchy"""
    ne = len(H.mMeshes[k].mElements)
    return H.mStiffness[k].shape[0] // ne, ne


def with_patch_smoothers(o, H, levels, width=2, hybrid=True):
    """a copy of the oracle hierarchy H with the element-patch smoother on `levels`"""
    H2 = copy.copy(H)
    H2.mSmoothers = list(H.mSmoothers)
    for k in levels:
        m, ne = level_shape(H, k)
        H2.mSmoothers[k] = oracle_patch_smoother(o, H.mStiffness[k], m, ne, width, hybrid)
    return H2


def cycles_to_tol(o, H, b, nPre=3, nPost=3, alpha=2.0 / 3.0, tol=1e-8, maxiter=400):
    """V(nPre, nPost) cycles from the zero guess until ||A x - b|| < tol ||b|| (the loop of src/solvers.jl:116-139)"""
    A = H.mStiffness[0]
    x = np.zeros(len(b))
    nb = np.linalg.norm(b)
    for it in range(1, maxiter + 1):
        x = o.multigrid_v_cycle(H, x, b, nPre, nPost, alpha)
        res = np.linalg.norm(o.csc_matvec(A, x) - b)
        if not np.isfinite(res):
            return maxiter + 1
        if res < tol * nb:
            return it
    return maxiter + 1


class BlockTridiag:
    """a hand-shaped block-tridiagonal operator of ne elements of m rows: sub[e] (couples e to e - 1), diag[e], sup[e]
    (e to e + 1) as (ne, m, m) arrays (sub[0] and sup[ne - 1] are not part of the operator), and the sweep of the
    definition above in float64, vectorised over the elements"""

    def __init__(self, sub, diag, sup):
        self.sub, self.diag, self.sup = (np.array(x, dtype=np.float64) for x in (sub, diag, sup))
        self.ne, self.m = self.diag.shape[:2]
        self.sub[0] = 0.0
        self.sup[-1] = 0.0
        self._zinv = None

    def tocsc(self):
        import scipy.sparse as sp
        ne, m = self.ne, self.m
        e, i, j = np.meshgrid(np.arange(ne), np.arange(m), np.arange(m), indexing="ij")
        rows, cols, vals = [], [], []
        for blk, off in ((self.diag, 0), (self.sub, -1), (self.sup, 1)):
            keep = (e + off >= 0) & (e + off < ne)
            rows.append((e * m + i)[keep])
            cols.append(((e + off) * m + j)[keep])
            vals.append(blk[keep])
        A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(ne * m, ne * m)).tocsc()
        A.eliminate_zeros()
        A.sort_indices()
        return A

    def matvec(self, u):
        U = u.reshape(self.ne, self.m)
        Y = np.einsum("eij,ej->ei", self.diag, U)
        Y[1:] += np.einsum("eij,ej->ei", self.sub[1:], U[:-1])
        Y[:-1] += np.einsum("eij,ej->ei", self.sup[:-1], U[1:])
        return Y.reshape(-1)

    def patch_blocks(self):
        """(ne - 1, 2m, 2m): A[P_e, P_e]"""
        m = self.m
        B = np.zeros((self.ne - 1, 2 * m, 2 * m))
        B[:, :m, :m] = self.diag[:-1]
        B[:, m:, m:] = self.diag[1:]
        B[:, :m, m:] = self.sup[:-1]
        B[:, m:, :m] = self.sub[1:]
        return B

    def sweep(self, u, b, w, hybrid=True):
        ne, m = self.ne, self.m
        r = (b - self.matvec(u)).reshape(ne, m)
        t = np.zeros((ne, m))
        if ne == 1:
            t[0] = np.linalg.solve(self.diag[0], r[0])
        else:
            if self._zinv is None:
                self._zinv = np.linalg.inv(self.patch_blocks())
            y = np.einsum("eij,ej->ei", self._zinv, np.concatenate([r[:-1], r[1:]], axis=1))
            t[:-1] += y[:, :m]
            t[1:] += y[:, m:]
            if hybrid:
                t[1:-1] *= 0.5
        return u + w * t.reshape(-1)

    def sweeps(self, u, b, weights, hybrid=True):
        for w in weights:
            u = self.sweep(u, b, w, hybrid)
        return u


def random_block_tridiag(m, ne, coupling, seed):
    """random, NON-uniform, diagonally dominant block-tridiagonal operator with symmetric positive definite diagonal
    blocks.  coupling: 'dense' (full off-diagonal blocks, A symmetric), 'row' (Sup_e one non-zero row m - 1 and
    Sub_e = Sup_{e-1}' one non-zero column: A symmetric, the pattern of a DG flux operator), 'rowcol' (Sup_e one non-zero row 1
    and Sub_e one non-zero column 0 with values of their own: A not symmetric; m >= 2)"""
    rng = np.random.default_rng(seed)
    sup = np.zeros((ne, m, m))
    sub = np.zeros((ne, m, m))
    if coupling == "dense":
        sup[:] = rng.uniform(-1.0, 1.0, (ne, m, m))
        sub[1:] = np.transpose(sup[:-1], (0, 2, 1))
    elif coupling == "row":
        sup[:, m - 1, :] = rng.uniform(-1.0, 1.0, (ne, m))
        sub[1:] = np.transpose(sup[:-1], (0, 2, 1))
    elif coupling == "rowcol":
        sup[:, 1, :] = rng.uniform(-1.0, 1.0, (ne, m))
        sub[:, :, 0] = rng.uniform(-1.0, 1.0, (ne, m))
    else:
        raise ValueError(coupling)
    R = rng.uniform(-1.0, 1.0, (ne, m, m))
    diag = 0.5 * (R + np.transpose(R, (0, 2, 1)))
    T = BlockTridiag(sub, diag, sup)
    off = np.abs(T.sub).sum(axis=2) + np.abs(T.sup).sum(axis=2) + np.abs(diag).sum(axis=2)   # (ne, m) row sums
    shift = off.max(axis=1) * rng.uniform(1.2, 3.0, ne)                                       # a different scale per element
    T.diag += shift[:, None, None] * np.eye(m)[None]
    return T
