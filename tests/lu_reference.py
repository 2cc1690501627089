"""The LU reference of the set-up tests (test_gpu_setup.py, test_gpu_setup_unstructured.py): partial-pivot LU in LAPACK
getf2 order, then the inverse column by column -- the operation sequence of lu_invert / block_invert_any_kernel in
csrc/setup_kernels.hpp, one IEEE operation at a time (NumPy float64 scalars: no contraction)."""
import numpy as np


class SingularAtStep(ZeroDivisionError):
    """the pivot of elimination step `step` (0-based) is exactly zero"""

    def __init__(self, step):
        super().__init__(f"zero pivot at elimination step {step}")
        self.step = step


def getf2_factor(a, steps=None):
    """-> (lu, piv, ties): L (unit diagonal, below) and U in one array, piv[k] = row exchanged with row k at step k (the
    FIRST row of largest |a[i, k]|, i >= k, as np.argmax picks it), ties = the steps at which more than one row attained
    that maximum (an observation for the tests; nothing computed depends on it).  steps: stop after that many elimination
    steps (the working array as the next step's pivot search sees it)"""
    m = a.shape[0]
    a = a.copy()
    piv = [0] * m
    ties = []
    for k in range(m if steps is None else steps):
        col = np.abs(a[k:, k])
        p = k + int(np.argmax(col))
        piv[k] = p
        if np.count_nonzero(col == col[p - k]) > 1:
            ties.append(k)
        if a[p, k] == 0.0:
            raise SingularAtStep(k)
        if p != k:
            a[[k, p], :] = a[[p, k], :]
        rp = 1.0 / a[k, k]
        for i in range(k + 1, m):
            a[i, k] *= rp
        for i in range(k + 1, m):
            l = a[i, k]
            for j in range(k + 1, m):
                a[i, j] -= l * a[k, j]
    return a, piv, ties


def getf2_inverse(a):
    """partial-pivot LU in LAPACK getf2 order, then the inverse column by column (the operation sequence of
    lu_invert in csrc/setup_kernels.hpp), plain Python floats"""
    m = a.shape[0]
    a, piv, _ = getf2_factor(a)
    inv = np.zeros((m, m))
    for c in range(m):
        x = np.zeros(m)
        x[c] = 1.0
        for k in range(m):
            if piv[k] != k:
                x[k], x[piv[k]] = x[piv[k]], x[k]
        for i in range(1, m):
            s = x[i]
            for j in range(i):
                s -= a[i, j] * x[j]
            x[i] = s
        for i in range(m - 1, -1, -1):
            s = x[i]
            for j in range(i + 1, m):
                s -= a[i, j] * x[j]
            x[i] = s / a[i, i]
        inv[:, c] = x
    return inv
