"""Right-preconditioned flexible GMRES(restart) around the oracle's V-cycle, in NumPy: the algorithm of the device loop
(aggmg_fgmres_dev), restated so that the two can be compared.  Test helper, not part of the package.

    M^-1 v = oracle.multigrid_v_cycle(H, 0, v, nPre, nPost, alpha),   A = H.mStiffness[0]

Every restart cycle starts from the explicit residual r = b - A x; inside a cycle, for j = 0, 1, ...: z_j = M^-1 v_j,
w = A z_j, h = V' w and w -= V h (classical Gram-Schmidt, one pass; mgs=True: modified Gram-Schmidt, one vector at a
time), h_{j+1,j} = ||w||, v_{j+1} = w / h_{j+1,j}.  The Hessenberg column goes through the Givens rotations of the
earlier columns and one of its own; res[it] = |g_{j+1}|.  Stop when it is < tol ||b||, at maxiter, when it is not
finite, or when ||w|| == 0; x += Z y at the end of every cycle and at the stop.
"""
import numpy as np


class Givens:
    """the least-squares part of one restart cycle: host_gmres.hpp, line for line"""

    def __init__(self, beta, m):
        self.R = np.zeros((m + 1, m))
        self.c = np.zeros(m)
        self.s = np.zeros(m)
        self.g = np.zeros(m + 1)
        self.g[0] = beta
        self.k = 0

    def push(self, h):
        j = self.k
        r = np.array(h[:j + 2], dtype=np.float64)
        for i in range(j):
            a, b = r[i], r[i + 1]
            r[i] = self.c[i] * a + self.s[i] * b
            r[i + 1] = self.c[i] * b - self.s[i] * a
        a, b = r[j], r[j + 1]
        d = float(np.hypot(a, b))
        if d == 0.0:
            self.c[j], self.s[j] = 1.0, 0.0
        else:
            self.c[j], self.s[j] = a / d, b / d
        r[j], r[j + 1] = d, 0.0
        self.R[:j + 2, j] = r
        self.g[j + 1] = -self.s[j] * self.g[j]
        self.g[j] = self.c[j] * self.g[j]
        self.k = j + 1
        return abs(self.g[self.k])

    def solve(self):
        k = self.k
        y = np.zeros(k)
        for i in range(k - 1, -1, -1):
            y[i] = (self.g[i] - self.R[i, i + 1:k] @ y[i + 1:k]) / self.R[i, i]
        return y


def fgmres_model(o, H, b, x0=None, restart=30, maxiter=200, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0, mgs=False,
                 cycle=None, kept=None):
    """-> (x, iter, res).  o: the oracle module, H: an oracle hierarchy.  cycle(v) replaces the oracle's V-cycle from a
    zero guess (e.g. one with a sweep-weight schedule).  kept: a list that receives (beta, Hbar, first) per restart
    cycle -- the Arnoldi matrix ((k + 1) x k) as the orthogonalisation produced it and the index of the cycle's first
    entry in res."""
    A = H.mStiffness[0]
    N = A.shape[0]
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(N) if x0 is None else np.array(x0, dtype=np.float64)
    zero = np.zeros(N)
    if cycle is None:
        def cycle(v):
            return o.multigrid_v_cycle(H, zero, v, nPre, nPost, alpha)
    nb = np.linalg.norm(b, 2)
    res = []
    done = False
    while not done and len(res) < maxiter:
        r = b - o.csc_matvec(A, x)
        beta = np.linalg.norm(r, 2)
        if beta == 0.0 or beta < tol * nb or not np.isfinite(beta):
            break
        m = min(restart, maxiter - len(res))
        V = np.zeros((N, m + 1))
        Z = np.zeros((N, m))
        Hbar = np.zeros((m + 1, m))
        V[:, 0] = r / beta
        ls = Givens(beta, m)
        first = len(res)
        finite = True
        for j in range(m):
            Z[:, j] = cycle(V[:, j])
            w = o.csc_matvec(A, Z[:, j])
            if mgs:
                for i in range(j + 1):
                    Hbar[i, j] = V[:, i] @ w
                    w = w - Hbar[i, j] * V[:, i]
            else:
                Hbar[:j + 1, j] = V[:, :j + 1].T @ w
                w = w - V[:, :j + 1] @ Hbar[:j + 1, j]
            Hbar[j + 1, j] = np.linalg.norm(w, 2)
            rj = ls.push(Hbar[:j + 2, j])
            res.append(float(rj))
            if not np.isfinite(rj):
                finite, done = False, True
                break
            if rj < tol * nb or Hbar[j + 1, j] == 0.0:
                done = True
                break
            if j + 1 < m:
                V[:, j + 1] = w / Hbar[j + 1, j]
        if kept is not None:
            kept.append((beta, Hbar[:ls.k + 1, :ls.k].copy(), first))
        if not finite:
            break
        x = x + Z[:, :ls.k] @ ls.solve()
    return x, len(res), res
