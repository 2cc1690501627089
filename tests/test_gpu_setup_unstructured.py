"""The device set-up algebra (csrc/spops.hip, csrc/setup_kernels.hpp, csrc/setup.hip) on unstructured patterns and on
blocks that pivot: sparse * sparse, sparse - sparse, BlockDiagonal * sparse, BlockDiagonalLU \\ sparse, the batched
pivoted LU -> explicit inverse (K6) through both of its entries, A[inds, inds] for arbitrary index lists, and the
validation of an uploaded SparseMatrixCSC.  tests/test_gpu_setup.py runs these kernels on what the hierarchy constructors
feed them; here every pattern is shaped by hand to reach one named branch.

References, all in this file (SciPy's product prunes and reorders: it is used for index patterns of positive matrices
only):
  * spmm_model / spsub_model / bdsp_model: the kernels' documented float64 operation sequence on CSC triples, one Python
    float operation at a time (CPython neither contracts nor reorders).  A device result has to equal its model BIT FOR
    BIT, index arrays included (`same_bits`: -0.0 is not 0.0 there);
  * an exact rational evaluation of the same products / block applies.  Every model entry lies within the running-error
    bound `gamma_n sum |a_i b_i|` of it (`entry_bound`) -- checked without a GPU, together with the self-tests of the
    comparison: models corrupted the way a kernel could be wrong (accumulation order swapped, one entry dropped from an
    insertion's shift, products fused into the additions) are rejected by `same_bits` on every case they can affect;
  * tests/lu_reference.py (getf2_factor / getf2_inverse) for the LU: device inverses equal it with == 0.0 difference;
    np.linalg is a sanity check only."""
import ctypes
import functools
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

from lu_reference import SingularAtStep, getf2_factor, getf2_inverse

U = Fraction(1, 2 ** 53)          # unit roundoff of float64, round to nearest
COL_CAP = 128                     # kColCap of csrc/spops.hip
THREADS = 256                     # kSetupThreads: one thread per column / per block


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


# ------------------------------------------------------------------------------------------
# CSC triples
# ------------------------------------------------------------------------------------------
class Csc:
    """the three arrays of a SparseMatrixCSC, 0-based, exactly as stored (zeros and all)"""

    def __init__(self, shape, indptr, indices, data):
        self.shape = (int(shape[0]), int(shape[1]))
        self.indptr = np.ascontiguousarray(indptr, dtype=np.int64)
        self.indices = np.ascontiguousarray(indices, dtype=np.int64)
        self.data = np.ascontiguousarray(data, dtype=np.float64)
        assert self.indptr.size == self.shape[1] + 1 and self.indptr[0] == 0 and self.indptr[-1] == self.indices.size
        assert self.indices.size == self.data.size

    @classmethod
    def from_columns(cls, shape, cols):
        """cols[j] = (rows, values) of column j, rows strictly ascending"""
        assert len(cols) == shape[1]
        for rows, vals in cols:
            assert len(rows) == len(vals) and all(0 <= r < shape[0] for r in rows)
            assert all(a < b for a, b in zip(rows[:-1], rows[1:]))
        indptr = np.concatenate(([0], np.cumsum([len(r) for r, _ in cols]))) if cols else np.zeros(1)
        indices = np.concatenate([np.asarray(r, dtype=np.int64) for r, _ in cols] + [np.zeros(0, dtype=np.int64)])
        data = np.concatenate([np.asarray(v, dtype=np.float64) for _, v in cols] + [np.zeros(0)])
        return cls(shape, indptr, indices, data)

    @classmethod
    def from_scipy(cls, M):
        M = sp.csc_matrix(M)
        M.sort_indices()
        return cls(M.shape, M.indptr, M.indices, M.data)

    @property
    def nnz(self):
        return int(self.data.size)

    def col(self, j):
        p, q = int(self.indptr[j]), int(self.indptr[j + 1])
        return [int(r) for r in self.indices[p:q]], [float(v) for v in self.data[p:q]]

    def scipy(self):
        return sp.csc_matrix((self.data.copy(), self.indices.copy(), self.indptr.copy()), shape=self.shape)

    def transposed(self):
        """the CSC arrays of the transpose: ascending rows inside a column, values copied"""
        m, n = self.shape
        cols = [([], []) for _ in range(m)]
        for j in range(n):
            for r, v in zip(*self.col(j)):
                cols[r][0].append(j)
                cols[r][1].append(v)
        return Csc.from_columns((n, m), cols)


def same_bits(G, W):
    """THE comparison of a device result with its model: shape, column pointers, row indices and the bits of the values"""
    return (G.shape == W.shape and np.array_equal(G.indptr, W.indptr) and np.array_equal(G.indices, W.indices)
            and np.array_equal(G.data.view(np.uint64), W.data.view(np.uint64)))


def upload(mg, T, kind=0, one_based=0):
    """a triple as a device operator, through the array entry (nothing of SciPy's in between)"""
    return mg.DeviceOperator((T.shape[0], T.shape[1], T.indptr + one_based, T.indices + one_based, T.data, one_based), kind)


def download(op):
    S = op.to_scipy()
    return Csc(S.shape, S.indptr, S.indices, S.data)


# ------------------------------------------------------------------------------------------
# models: the kernels' operation sequences in Python floats
# ------------------------------------------------------------------------------------------
class ColumnCapExceeded(Exception):
    pass


def _rounded_fma(acc, a, b):
    """acc + a * b with ONE rounding: what a contracted multiply-add would give"""
    return float(Fraction(acc) + Fraction(a) * Fraction(b))


def spmm_model(A, B, corrupt=None, stats=None):
    """spmm_kernel (csrc/spops.hip), as its header comment fixes it: for result column j the entries of B's column j in
    ascending row order k, inside each the entries of A's column k in ascending row order; a row met for the first time is
    inserted into the sorted thread-local list with accumulator 0.0 (the entries behind it shift up by one, rows[] and
    acc[] together), then acc += a * b with the product rounded first.  Nothing is pruned.  More than COL_CAP distinct
    rows in a column: ColumnCapExceeded (the kernel raises its error flag BEFORE it would write entry COL_CAP).
    corrupt: 'order' -- B's column walked in descending order; 'shift' -- the shift of acc[] stops one entry short (the
    accumulator at the insertion point is not moved up); 'fma' -- product and addition fused, one rounding.
    stats: dict, gets 'mid_inserts' (insertions in front of the end of the list) and 'max_terms'."""
    assert A.shape[1] == B.shape[0] and corrupt in (None, "order", "shift", "fma")
    cols = []
    mid, max_terms = 0, 0
    for j in range(B.shape[1]):
        rows, acc, terms = [], [], []
        brows, bvals = B.col(j)
        order = range(len(brows) - 1, -1, -1) if corrupt == "order" else range(len(brows))
        for q in order:
            bkj = bvals[q]
            arows, avals = A.col(brows[q])
            pos = 0
            for r, a in zip(arows, avals):
                while pos < len(rows) and rows[pos] < r:
                    pos += 1
                if pos == len(rows) or rows[pos] != r:
                    if len(rows) >= COL_CAP:
                        raise ColumnCapExceeded(j)
                    mid += pos < len(rows)
                    rows.append(0), acc.append(0.0), terms.append(0)
                    for s in range(len(rows) - 1, pos, -1):
                        rows[s], terms[s] = rows[s - 1], terms[s - 1]
                        if not (corrupt == "shift" and s == pos + 1):
                            acc[s] = acc[s - 1]
                    rows[pos], acc[pos], terms[pos] = r, 0.0, 0
                acc[pos] = _rounded_fma(acc[pos], a, bkj) if corrupt == "fma" else acc[pos] + a * bkj
                terms[pos] += 1
        cols.append((rows, acc))
        max_terms = max([max_terms] + terms)
    if stats is not None:
        stats.update(mid_inserts=mid, max_terms=max_terms)
    return Csc.from_columns((A.shape[0], B.shape[1]), cols)


def spsub_model(A, B, keep=lambda v: v != 0.0):
    """spsub_kernel: three-way merge of the two columns; a - b where both store the row, a or -b where one does; the
    result is stored iff v != 0.0 (so neither 0.0 nor -0.0 is ever stored)"""
    assert A.shape == B.shape
    cols = []
    for j in range(A.shape[1]):
        (ar, av), (br, bv) = A.col(j), B.col(j)
        pa = pb = 0
        rows, vals = [], []
        while pa < len(ar) or pb < len(br):
            if pb >= len(br) or (pa < len(ar) and ar[pa] < br[pb]):
                r, v = ar[pa], av[pa]
                pa += 1
            elif pa >= len(ar) or br[pb] < ar[pa]:
                r, v = br[pb], -bv[pb]
                pb += 1
            else:
                r, v = ar[pa], av[pa] - bv[pb]
                pa, pb = pa + 1, pb + 1
            if keep(v):
                rows.append(r), vals.append(v)
        cols.append((rows, vals))
    return Csc.from_columns(A.shape, cols)


def bdsp_model(blocks, S, corrupt=None):
    """bdsp_count_kernel / bdsp_fill_kernel: blocks (nb, m, m), block b = M[i, k]; per column of S and per touched block (in
    ascending order) the dense sub-vector t[0..m) (0.0 where S stores nothing), then for EVERY row i of the block
    acc = 0.0; acc += M[i, k] * t[k] over ALL k = 0..m-1 ascending, product rounded first; all m rows are emitted, zeros
    included.  corrupt: 'order' -- k descending; 'fma' -- one rounding per multiply-add."""
    nb, m, _ = blocks.shape
    assert S.shape[0] == nb * m and corrupt in (None, "order", "fma")
    cols = []
    for j in range(S.shape[1]):
        srows, svals = S.col(j)
        rows, vals = [], []
        p = 0
        while p < len(srows):
            b = srows[p] // m
            t = [0.0] * m
            while p < len(srows) and srows[p] // m == b:
                t[srows[p] - b * m] = svals[p]
                p += 1
            for i in range(m):
                acc = 0.0
                for k in (range(m - 1, -1, -1) if corrupt == "order" else range(m)):
                    mik = float(blocks[b, i, k])
                    acc = _rounded_fma(acc, mik, t[k]) if corrupt == "fma" else acc + mik * t[k]
                rows.append(b * m + i), vals.append(acc)
        cols.append((rows, vals))
    return Csc.from_columns(S.shape, cols)


# ------------------------------------------------------------------------------------------
# exact references and the bound
# ------------------------------------------------------------------------------------------
def gamma(n):
    return n * U / (1 - n * U)


def entry_bound(nterms, S):
    """Bound on |model entry - exact entry| for an entry accumulated from `nterms` products, u = 2^-53.

    Every float64 operation returns its exact result times (1 + d), |d| <= u (no overflow; the values of these tests are
    far from the subnormal range, except where a test says so and then the operations involved are exact).  An entry is
    computed as  acc = 0.0;  acc = fl(acc + fl(a_i b_i)), i = 1..t:  t multiplications and t additions.  Product i passes
    through its own rounding and through the additions i..t, at most t of them, so the computed value is
    sum_i a_i b_i (1 + e_i) with (1 + e_i) a product of at most t + 1 <= 2t factors (1 + d), i.e. |e_i| <= gamma_2t, and

        |computed - sum_i a_i b_i| <= gamma_n sum_i |a_i b_i|,      n = 2t = products + additions,
                                                                     gamma_n = n u / (1 - n u).

    (t + 1 would do; n counts every operation performed, first addition to 0.0 included.)  A term with a_i b_i = 0 adds
    nothing to either side, so a block apply over all m entries of the gathered sub-vector has t = m whatever the column
    stores.  The bound holds for every order of the additions and for fused multiply-adds alike: it says that the model is
    the stated sum and not another one (an entry left out, moved to another row or added twice is off by about a whole
    term, ~2^50 bounds); the ORDER is pinned by the bit comparison, not by this.  Nothing measured enters it."""
    return gamma(2 * nterms) * S


def spmm_exact(A, B):
    """per result column {row: (exact sum, sum of |products|, number of products)}"""
    fa = [Fraction(float(v)) for v in A.data]
    out = []
    for j in range(B.shape[1]):
        col = {}
        for k, b in zip(*B.col(j)):
            fb = Fraction(b)
            for p in range(int(A.indptr[k]), int(A.indptr[k + 1])):
                r = int(A.indices[p])
                s, S, t = col.get(r, (Fraction(0), Fraction(0), 0))
                col[r] = (s + fa[p] * fb, S + abs(fa[p] * fb), t + 1)
        out.append(col)
    return out


def bdsp_exact(blocks, S):
    nb, m, _ = blocks.shape
    out = []
    for j in range(S.shape[1]):
        col = {}
        srows, svals = S.col(j)
        for b in sorted({r // m for r in srows}):
            t = {r - b * m: Fraction(v) for r, v in zip(srows, svals) if r // m == b}
            for i in range(m):
                s, Sabs = Fraction(0), Fraction(0)
                for k, tk in t.items():
                    prod = Fraction(float(blocks[b, i, k])) * tk
                    s, Sabs = s + prod, Sabs + abs(prod)
                col[b * m + i] = (s, Sabs, m)
        out.append(col)
    return out


def outside_bound(C, exact):
    """(column, row) of every entry of the triple C that the exact reference does not have, misses, or has further away
    than entry_bound"""
    bad = []
    for j, col in enumerate(exact):
        rows, vals = C.col(j)
        if rows != sorted(col):
            bad.append((j, None))
            continue
        for r, v in zip(rows, vals):
            s, S, t = col[r]
            if not np.isfinite(v) or abs(Fraction(v) - s) > entry_bound(t, S):
                bad.append((j, r))
    return bad


# ------------------------------------------------------------------------------------------
# values and random patterns
# ------------------------------------------------------------------------------------------
def _values(rng, n):
    """either sign, 53-bit mantissas (products of two are inexact), magnitudes over 13 binades"""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-6, 7, n)


def random_csc(rng, m, n, lo=2, hi=6, empty=(), zero_every=7, local=0):
    """about 4 entries per column at random rows; columns in `empty` store nothing; every zero_every-th stored value is 0.0.
    local > 0: about half of a column's rows come from a window of that many rows at the column's relative position (so
    that the columns a product merges share rows: entries of three and more products), the rest from anywhere"""
    cols = []
    for j in range(n):
        k = 0 if j in empty else min(m, int(rng.integers(lo, hi + 1)))
        rows = set()
        while len(rows) < k:
            if local and rng.random() < 0.5:
                rows.add(min(m - 1, j * m // n + int(rng.integers(0, local))))
            else:
                rows.add(int(rng.integers(0, m)))
        cols.append((sorted(rows), _values(rng, k)))
    T = Csc.from_columns((m, n), cols)
    if zero_every:
        T.data[::zero_every] = 0.0
    return T


def dense_csc(rng, m, n):
    return Csc.from_columns((m, n), [(list(range(m)), _values(rng, m)) for _ in range(n)])


# ------------------------------------------------------------------------------------------
# 1. sparse product
# ------------------------------------------------------------------------------------------
ORDER_TERMS = [1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53]
# added from 0.0 in this order every 2^-53 is half an ulp of 1.0 and is rounded away (ties to even): 1.0; in the opposite
# order the four of them make 2^-51 first: 1.0 + 2^-51


def _p_random_rect(rng):
    return random_csc(rng, 301, 203, local=6), random_csc(rng, 203, 517, local=6)


def _p_empty_columns(rng):
    """B: empty first and last column, all of workgroup 1 (columns 256..511) and a few more; A: empty columns that B's
    columns select -- column 1 of B selects nothing else (a stored column with an empty result)"""
    a_empty = (0, 5, 100, 202)
    A = random_csc(rng, 301, 203, empty=a_empty, local=6)
    b_empty = {0, 699, 7, 255, 512} | set(range(256, 512))
    cols = []
    for j in range(700):
        if j in b_empty:
            cols.append(([], []))
        elif j == 1:
            cols.append((list(a_empty), _values(rng, 4)))
        else:
            rows = {int(rng.integers(0, 203))} | set(min(202, j * 203 // 700 + int(r)) for r in rng.integers(0, 6, 4))
            if j % 3 == 0:
                rows.add(a_empty[j % 4])
            cols.append((sorted(rows), _values(rng, len(rows))))
    return A, Csc.from_columns((203, 700), cols)


def _p_tiny(m, k, n):
    def build(rng):
        A, B = dense_csc(rng, m, k), dense_csc(rng, k, n)
        if (m, k, n) == (1, 7, 1):
            # one entry of 7 products: -1, fl(1/3) * 3 = 1 - 2^-54 (rounds to 1.0), 2^-53 four times, 2^-60.  In this order
            # 2^-51 + 2^-60; descending, 2^-60 and the 2^-53's vanish in 1.0: 2^-51; fused, -1 + (1 - 2^-54) survives
            A.data[:] = [-0.5, 1.0 / 3.0, 2.0 ** -50, 2.0 ** -51, 2.0 ** -52, 2.0 ** -51, 2.0 ** -60]
            B.data[:] = [2.0, 3.0, 2.0 ** -3, 2.0 ** -2, 2.0 ** -1, 2.0 ** -2, 1.0]
        return A, B
    return build


def _p_zero_columns(rng):
    return random_csc(rng, 5, 3), Csc.from_columns((3, 0), [])


def _p_insert_front(rng):
    """column k of A holds the single row 11 - k: with B's column selecting k = 0, 1, 2, ... every insertion is at
    position 0 and shifts the whole list"""
    K = 12
    A = Csc.from_columns((K, K), [([K - 1 - k], _values(rng, 1)) for k in range(K)])
    B = Csc.from_columns((K, 3), [(list(range(K)), _values(rng, K)), (list(range(0, K, 2)), _values(rng, K // 2)),
                                  ([3], _values(rng, 1))])
    return A, B


def _p_insert_front_blocks(rng):
    """column k of A holds three rows, all above (smaller than) those of column k - 1: runs inserted at positions 0, 1, 2"""
    K = 9
    A = Csc.from_columns((3 * K, K), [([3 * (K - 1 - k) + i for i in range(3)], _values(rng, 3)) for k in range(K)])
    B = Csc.from_columns((K, 2), [(list(range(K)), _values(rng, K)), ([1, 4, 8], _values(rng, 3))])
    return A, B


def _p_interleave(rng):
    """A's columns hold the rows of one residue mod 4 (0, 1, 2, 3, then 2, 0, 3, 1): insertions all over the list"""
    res = [0, 1, 2, 3, 2, 0, 3, 1]
    A = Csc.from_columns((40, 8), [(list(range(r, 40, 4)), _values(rng, 10)) for r in res])
    B = Csc.from_columns((8, 4), [([0, 1, 2, 3], _values(rng, 4)), ([4, 5, 6, 7], _values(rng, 4)),
                                  (list(range(8)), _values(rng, 8)), ([1, 6], _values(rng, 2))])
    return A, B


def _p_full_overlap(rng):
    """five columns of A with the same six rows, all selected by one column of B: nothing but accumulation, five products
    per entry.  Row 0 gets the products ORDER_TERMS exactly in B's column 0 (B's values are powers of two there, A's the
    terms divided by them); the second stored row with B's column 1: -0.5 * 2, fl(1/3) * 3 = 1 - 2^-54, then stored zeros --
    0.0 with rounded products, -2^-54 with fused ones"""
    rows = [1, 4, 5, 9, 10, 13]
    bvals = [1.0, 2.0, 0.5, 4.0, 0.25]
    cols = []
    for k in range(5):
        v = _values(rng, 6)
        v[0] = ORDER_TERMS[k] / bvals[k]
        v[1] = [-0.5, 1.0 / 3.0, 0.0, 0.0, 0.0][k]
        cols.append((rows, v))
    return Csc.from_columns((14, 5), cols), Csc.from_columns((5, 2), [(list(range(5)), bvals), (list(range(5)), [2.0, 3.0, 1.0, 1.0, 1.0])])


def _cap_A(rng):
    """200 x 4: columns of 50 + 50 + 28 disjoint, interleaved rows, and a fourth column with one more row"""
    return Csc.from_columns((200, 4), [(list(range(0, 200, 4)), _values(rng, 50)), (list(range(1, 200, 4)), _values(rng, 50)),
                                       (list(range(2, 112, 4)), _values(rng, 28)), ([199], _values(rng, 1))])


def _p_cap_128(rng):
    A = _cap_A(rng)
    return A, Csc.from_columns((4, 3), [([0, 1, 2], _values(rng, 3)), ([3], _values(rng, 1)), ([2, 3], _values(rng, 2))])


def _p_cap_129(rng):
    A = _cap_A(rng)
    return A, Csc.from_columns((4, 3), [([0, 1, 2], _values(rng, 3)), ([0, 1, 2, 3], _values(rng, 4)), ([3], _values(rng, 1))])


# name -> (builder, seed, corruptions of the model that change its bits on this case)
PRODUCTS = {
    "random_rect": (_p_random_rect, 101, {"order", "shift", "fma"}),
    "empty_columns": (_p_empty_columns, 102, {"order", "shift", "fma"}),
    "1x1.1x1": (_p_tiny(1, 1, 1), 103, set()),
    "1x7.7x1": (_p_tiny(1, 7, 1), 104, {"order", "fma"}),
    "7x1.1x7": (_p_tiny(7, 1, 7), 105, set()),
    "zero_columns": (_p_zero_columns, 106, set()),
    "insert_front": (_p_insert_front, 107, {"shift"}),
    "insert_front_blocks": (_p_insert_front_blocks, 108, {"shift"}),
    "interleave": (_p_interleave, 109, {"shift", "fma"}),
    "full_overlap": (_p_full_overlap, 110, {"order", "fma"}),
    "cap_128": (_p_cap_128, 111, {"shift"}),
}


@functools.lru_cache(maxsize=None)
def product_case(name):
    build, seed, sens = PRODUCTS[name]
    A, B = build(np.random.default_rng(seed))
    stats = {}
    return A, B, spmm_model(A, B, stats=stats), stats, sens


def aggregation(rng, n):
    """piecewise-constant aggregation, ragged aggregates of 1 .. 5 rows, under a random row permutation (as
    tests/test_gpu_generic_csr.py builds its transfers)"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 6)))
    sizes[-1] -= sum(sizes) - n
    agg = np.repeat(np.arange(len(sizes)), sizes)
    return Csc.from_scipy(sp.csc_matrix((np.ones(n), (rng.permutation(n), agg)), shape=(n, len(sizes)))), sizes


@functools.lru_cache(maxsize=None)
def galerkin_case():
    rng = np.random.default_rng(120)
    n = 150
    L, sizes = aggregation(rng, n)
    R = random_csc(rng, n, n, lo=4, hi=8, zero_every=0).scipy()
    X = Csc.from_scipy(R + R.T)
    Lt = L.transposed()
    LtX = spmm_model(Lt, X)
    return L, sizes, X, Lt, LtX, spmm_model(LtX, L)


def test_product_cases_reach_their_branches():
    """no GPU: what the case table claims about its patterns, from the patterns themselves"""
    A, B, C, st, _ = product_case("random_rect")
    assert A.shape == (301, 203) and B.shape == (203, 517) and B.shape[1] > 2 * THREADS and B.shape[1] % THREADS
    for T in (A, B):
        assert np.all(T.data[::7] == 0.0) and np.count_nonzero(T.data == 0.0) == len(T.data[::7])
        mags = np.abs(T.data[T.data != 0.0])
        assert (T.data < 0).any() and (T.data > 0).any() and mags.max() / mags.min() > 2.0 ** 10
        assert 3.5 < T.nnz / T.shape[1] < 4.5
    assert st["mid_inserts"] > 100 and st["max_terms"] >= 3
    A, B, C, st, _ = product_case("empty_columns")
    blen, alen, clen = np.diff(B.indptr), np.diff(A.indptr), np.diff(C.indptr)
    assert blen[0] == 0 and blen[-1] == 0 and np.all(blen[THREADS:2 * THREADS] == 0) and B.shape[1] > 2 * THREADS
    assert np.count_nonzero(alen == 0) == 4 and all(np.any(B.indices == k) for k in np.nonzero(alen == 0)[0])
    assert blen[1] == 4 and clen[1] == 0                       # a stored column of B that selects empty columns only
    A, B, C, st, _ = product_case("insert_front")
    assert st["mid_inserts"] == 11 + 5 and C.col(0)[0] == list(range(12))
    A, B, C, st, _ = product_case("insert_front_blocks")
    assert st["mid_inserts"] == 3 * 8 + 3 * 2 and C.col(0)[0] == list(range(27))
    A, B, C, st, _ = product_case("interleave")
    assert st["mid_inserts"] >= 60 and C.col(2)[0] == list(range(40)) and st["max_terms"] == 2
    A, B, C, st, _ = product_case("full_overlap")
    assert st["mid_inserts"] == 0 and st["max_terms"] == 5 and C.nnz == 12
    # the order-sensitive row: ascending and descending sums differ in the last bits -- on the model, so the case
    # cannot go vacuous
    prods = [a * b for a, b in zip([A.col(k)[1][0] for k in range(5)], B.col(0)[1])]
    assert prods == ORDER_TERMS
    up = functools.reduce(lambda s, p: s + p, prods, 0.0)
    down = functools.reduce(lambda s, p: s + p, prods[::-1], 0.0)
    assert up == 1.0 and down == 1.0 + 2.0 ** -51
    assert C.col(0)[1][0] == up and spmm_model(A, B, "order").col(0)[1][0] == down
    assert C.col(1)[1][1] == 0.0 and spmm_model(A, B, "fma").col(1)[1][1] == -2.0 ** -54
    A, B, C, st, _ = product_case("cap_128")
    assert [len(A.col(k)[0]) for k in range(4)] == [50, 50, 28, 1]
    assert len(set(A.indices.tolist())) == 129 and np.diff(C.indptr).tolist() == [COL_CAP, 1, 29]
    A, B = _p_cap_129(np.random.default_rng(111))
    with pytest.raises(ColumnCapExceeded):
        spmm_model(A, B)
    L, sizes, X, Lt, LtX, C = galerkin_case()
    assert set(sizes) == {1, 2, 3, 4, 5} and np.all(np.diff(Lt.indptr) == 1)
    assert np.array_equal(X.scipy().toarray(), X.scipy().toarray().T) and 9 < X.nnz / X.shape[0] < 13


def _ones(T):
    S = T.scipy()
    S.data[:] = 1.0
    return S


@pytest.mark.parametrize("name", list(PRODUCTS))
def test_product_model_against_exact_reference(name):
    """no GPU: the model's index arrays are the pattern of the Boolean product (stored zeros are entries: nothing pruned,
    nothing missing); every model entry lies within entry_bound of the exact rational entry; each corrupted model changes
    the bits on exactly the cases the table lists (and only a case with insertions in front of the list's end can list
    'shift', only one with three or more products in an entry 'order'); the model with the broken shift also leaves the
    bound -- an entry it loses is a whole term, not a rounding."""
    A, B, C, st, sens = product_case(name)
    P = sp.csc_matrix(_ones(A) @ _ones(B))
    P.sort_indices()
    assert np.array_equal(P.indptr, C.indptr) and np.array_equal(P.indices, C.indices)
    exact = spmm_exact(A, B)
    assert outside_bound(C, exact) == []
    assert ("shift" in sens) == (st["mid_inserts"] > 0)
    assert "order" not in sens or st["max_terms"] >= 3
    assert "fma" not in sens or st["max_terms"] >= 2
    for corrupt in ("order", "shift", "fma"):
        W = spmm_model(A, B, corrupt)
        assert same_bits(W, C) == (corrupt not in sens), corrupt
        assert np.array_equal(W.indptr, C.indptr) and np.array_equal(W.indices, C.indices)
        if corrupt == "shift" and corrupt in sens:
            assert outside_bound(W, exact) != []
        if corrupt in ("order", "fma"):
            assert outside_bound(W, exact) == []       # (the bound does not see the order: the bit comparison does)


def test_galerkin_model_against_exact_reference():
    """no GPU: both stages of L' X L within the bound of their exact products (the second one of the exact product of
    the first stage's float64 values: it is that stage's input)"""
    L, sizes, X, Lt, LtX, C = galerkin_case()
    assert outside_bound(LtX, spmm_exact(Lt, X)) == []
    assert outside_bound(C, spmm_exact(LtX, L)) == []
    stats = {}
    spmm_model(LtX, L, stats=stats)
    assert stats["mid_inserts"] > 0 and stats["max_terms"] >= 3
    for corrupt in ("order", "shift"):
        assert not same_bits(spmm_model(spmm_model(Lt, X, corrupt), L, corrupt), C), corrupt
    # (every product has a factor 1.0 and is exact: fusing it into the addition changes nothing here)
    assert same_bits(spmm_model(spmm_model(Lt, X, "fma"), L, "fma"), C)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PRODUCTS))
def test_sparse_product_bits(mg, name):
    A, B, C, _, _ = product_case(name)
    got = download(upload(mg, A).matmul(upload(mg, B)))
    assert same_bits(got, C), name


@pytest.mark.gpu
def test_sparse_product_column_cap(mg):
    """a result column of exactly kColCap = 128 rows is computed; one of 129 is refused with UnsupportedError naming the
    limit (the kernel tests `len >= kColCap` before it writes entry 128 of its thread-local arrays); the refusal leaves
    nothing behind: the same context computes the 128-row product again"""
    A, B, C, _, _ = product_case("cap_128")
    dA = upload(mg, A)
    assert same_bits(download(dA.matmul(upload(mg, B))), C)
    A9, B9 = _p_cap_129(np.random.default_rng(111))
    assert same_bits(A9, A)
    with pytest.raises(mg.UnsupportedError, match=r"more than 128 rows"):
        dA.matmul(upload(mg, B9))
    assert same_bits(download(dA.matmul(upload(mg, B))), C)


@pytest.mark.gpu
def test_galerkin_chain_bits(mg):
    """Lt.matmul(X).matmul(L) with Lt the device transposition of a ragged, row-permuted aggregation: the bits of the
    model applied twice (and the transposition itself: the CSC arrays of L')"""
    L, sizes, X, Lt, LtX, C = galerkin_case()
    dL = upload(mg, L, kind=1)
    dLt = dL.transpose()
    assert same_bits(download(dLt), Lt)
    mid = dLt.matmul(upload(mg, X))
    assert same_bits(download(mid), LtX)
    assert same_bits(download(mid.matmul(dL)), C)


# ------------------------------------------------------------------------------------------
# 2. sparse difference
# ------------------------------------------------------------------------------------------
TINY = 1e-305                      # nonzero, below any "is it small" threshold a wrong kernel might use
UP = float(np.nextafter(1.0, 2.0))


@functools.lru_cache(maxsize=None)
def sub_case():
    """12 x 257; columns 0 .. 8 by hand (see test_difference_model_on_the_hand_built_columns), 9 .. 255 random pairs
    sharing about half of their rows, column 256 -- alone in the last workgroup -- stored in A only"""
    rng = np.random.default_rng(130)
    z = 0.0
    a = [([1, 4, 7], [1.5, -2.5, 3.5]),                              # 0: stored in A only
         ([], []),                                                   # 1: stored in B only
         ([0, 2, 4, 6], [1.0, 2.0, 3.0, 4.0]),                       # 2: rows interleaved
         ([0, 3, 5, 8, 9], [1.0, 1.0, -3.0, 1e-300, 0.1]),           # 3: rows identical
         ([], []),                                                   # 4: stored in neither
         ([2, 7, 8, 9, 10], [z, z, z, -z, 2.0]),                     # 5: stored zeros
         ([0, 1, 5, 9, 11], [1.0, 2.0, 3.0, 4.0, 5.0]),              # 6: partial overlap, both tails
         ([3], [TINY]),                                              # 7: tiny but nonzero
         ([0, 1, 2], [5.0, 6.0, 7.0])]                               # 8: A's rows all before B's
    b = [([], []),
         ([0, 11], [1.5, -2.5]),
         ([1, 3, 5, 7], [1.0, 2.0, 3.0, 4.0]),
         ([0, 3, 5, 8, 9], [1.0, UP, -3.0, float(np.nextafter(1e-300, 1.0)), 0.1]),
         ([], []),
         ([5, 7, 8, 10], [z, z, 3.0, 2.0]),
         ([1, 2, 5, 10, 11], [2.0, 7.0, 1.0, 8.0, 5.0]),
         ([6], [-TINY]),
         ([9, 10, 11], [5.0, 6.0, 7.0])]
    for j in range(9, 256):
        ra = sorted(int(r) for r in rng.choice(12, size=int(rng.integers(0, 7)), replace=False))
        rb = sorted(set(r for r in ra if rng.random() < 0.5) | set(int(r) for r in rng.choice(12, size=int(rng.integers(0, 4)), replace=False)))
        va, vb = _values(rng, len(ra)), _values(rng, len(rb))
        for i, r in enumerate(rb):                                   # every third shared row: equal values
            if r in ra and (r + j) % 3 == 0:
                vb[i] = va[ra.index(r)]
        a.append((ra, va))
        b.append((rb, vb))
    a.append(([0, 6, 11], [1.0, -2.0, 3.0]))
    b.append(([], []))
    A, B = Csc.from_columns((12, 257), a), Csc.from_columns((12, 257), b)
    return A, B, spsub_model(A, B)


def test_difference_model_on_the_hand_built_columns():
    """no GPU: what the three-way merge has to give on the hand-built columns, written out; and that the model is
    sensitive to the two ways a drop test can be wrong (a threshold instead of != 0.0; none at all)"""
    A, B, C = sub_case()
    assert A.shape[1] == THREADS + 1
    assert C.col(0) == ([1, 4, 7], [1.5, -2.5, 3.5])
    assert C.col(1) == ([0, 11], [-1.5, 2.5])
    assert C.col(2) == ([0, 1, 2, 3, 4, 5, 6, 7], [1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 4.0, -4.0])
    # equal entries go; entries one ulp apart stay, with a - b exactly (both differences are exact: Sterbenz)
    d300 = 1e-300 - float(np.nextafter(1e-300, 1.0))
    assert C.col(3) == ([3, 8], [-2.0 ** -52, d300]) and d300 != 0.0 and abs(d300) < 1e-315
    assert Fraction(d300) == Fraction(1e-300) - Fraction(float(np.nextafter(1e-300, 1.0)))
    assert C.col(4) == ([], [])
    # a stored 0.0 of A alone, of B alone (-0.0), 0.0 - 0.0, -0.0 alone: all dropped; 0.0 - 3.0 and the cancelling 2.0 - 2.0
    assert C.col(5) == ([8], [-3.0])
    assert C.col(6) == ([0, 2, 5, 9, 10], [1.0, -7.0, 2.0, 4.0, -8.0])
    assert C.col(7) == ([3, 6], [TINY, TINY])
    assert C.col(8) == ([0, 1, 2, 9, 10, 11], [5.0, 6.0, 7.0, -5.0, -6.0, -7.0])
    assert C.col(256) == ([0, 6, 11], [1.0, -2.0, 3.0])
    assert not np.any(C.data == 0.0)
    shared = sum(len(set(A.col(j)[0]) & set(B.col(j)[0])) for j in range(9, 256))
    dropped = sum(len(set(A.col(j)[0]) | set(B.col(j)[0])) for j in range(257)) - C.nnz
    assert shared > 150 and dropped > 40
    assert not same_bits(spsub_model(A, B, keep=lambda v: abs(v) > 1e-300), C)
    assert not same_bits(spsub_model(A, B, keep=lambda v: True), C)


@pytest.mark.gpu
def test_sparse_difference_bits(mg):
    A, B, C = sub_case()
    assert same_bits(download(upload(mg, A).sub(upload(mg, B))), C)
    assert same_bits(download(upload(mg, B).sub(upload(mg, A))), spsub_model(B, A))


@pytest.mark.gpu
def test_sparse_difference_all_cancelling(mg):
    """A - A over 513 columns (two full workgroups and one column): no entry, a valid all-zero column pointer"""
    A = random_csc(np.random.default_rng(131), 40, 513)
    dA = upload(mg, A)
    Z = download(dA.sub(upload(mg, A)))
    assert Z.shape == (40, 513) and Z.nnz == 0 and Z.indptr.size == 514 and not Z.indptr.any()
    assert same_bits(Z, spsub_model(A, A))
    Z = download(dA.sub(dA))
    assert Z.nnz == 0 and not Z.indptr.any()


# ------------------------------------------------------------------------------------------
# 3. BlockDiagonal * sparse, BlockDiagonalLU \ sparse
# ------------------------------------------------------------------------------------------
BD_SHAPES = [(1, 40), (2, 30), (5, 12), (5, 1), (8, 9), (9, 7), (16, 6), (33, 6), (64, 6), (64, 1)]   # (m, nb): m nb < 1500


@functools.lru_cache(maxsize=None)
def reference_inverse(block_bytes, m):
    return getf2_inverse(np.frombuffer(block_bytes).reshape(m, m))


def inverses(blocks):
    m = blocks.shape[1]
    return np.stack([reference_inverse(np.ascontiguousarray(b).tobytes(), m) for b in blocks])


@functools.lru_cache(maxsize=None)
def bd_case(m, nb):
    """blocks: identity-dominated with entries of either sign (condition number far below 100), every other one with its
    rows reversed (its LU exchanges rows); S: one column per branch, see the assertions of
    test_block_apply_model_against_exact_reference"""
    rng = np.random.default_rng(1000 * m + nb)
    blocks = np.stack([2.0 * np.eye(m) + rng.uniform(-1.0, 1.0, (m, m)) / m for _ in range(nb)])
    blocks[1::2] = blocks[1::2, ::-1, :].copy()
    if nb == 1:
        blocks = blocks[:, ::-1, :].copy()
    N = m * nb
    mid = nb // 2
    cols = [([m // 2], _values(rng, 1)),                                     # 0: one row, first block only
            ([N - 1], _values(rng, 1)),                                      # 1: last row of the last block only
            (sorted({b * m + i for b in (0, 2, 5) if b < nb for i in {0, m - 1}}), None),   # 2: non-adjacent blocks
            (list(range(mid * m, (mid + 1) * m)), None),                     # 3: all m rows of one block
            ([], []),                                                        # 4: empty
            (sorted({0, m - 1, N - m, N - 1}), 0.0),                         # 5: nothing but stored zeros
            (list(range(mid * m, (mid + 1) * m)), "mixed")]                  # 6: zeros among the rows of a block
    for _ in range(8):                                                       # 7 ..: random
        cols.append((sorted(int(r) for r in rng.choice(N, size=min(N, int(rng.integers(1, 7))), replace=False)), None))
    out = []
    for rows, vals in cols:
        if vals is None:
            vals = _values(rng, len(rows))
        elif isinstance(vals, float):
            vals = np.full(len(rows), vals)
        elif isinstance(vals, str):
            vals = _values(rng, len(rows))
            vals[::2] = 0.0
        out.append((rows, vals))
    S = Csc.from_columns((N, len(out)), out)
    return blocks, S, bdsp_model(blocks, S)


@pytest.mark.parametrize("m,nb", BD_SHAPES)
def test_block_apply_model_against_exact_reference(m, nb):
    """no GPU: the columns reach what they were built for; all m rows of every touched block are in the model, zeros
    included; every entry within entry_bound(m, .) of the exact block apply; the model with k descending differs in bits
    from m = 3 on, the fused one from m = 2 on (with fewer terms they cannot)"""
    blocks, S, C = bd_case(m, nb)
    assert m * nb < 1500 and max(np.linalg.cond(b) for b in blocks) < 100.0
    touched = [sorted({r // m for r in S.col(j)[0]}) for j in range(S.shape[1])]
    assert touched[0] == [0] and len(S.col(0)[0]) == 1
    assert touched[1] == [nb - 1] and S.col(1)[0] == [m * nb - 1]
    assert touched[2] == [b for b in (0, 2, 5) if b < nb] and (nb == 1 or len(touched[2]) == 3)
    assert len(S.col(3)[0]) == m and len(touched[3]) == 1
    assert touched[4] == [] and not np.any(S.col(5)[1]) and len(S.col(5)[0]) >= 1
    assert S.col(6)[1][0] == 0.0
    for j in range(S.shape[1]):
        assert C.col(j)[0] == [b * m + i for b in touched[j] for i in range(m)]
    assert C.col(5)[1] == [0.0] * (m * len(touched[5]))
    assert outside_bound(C, bdsp_exact(blocks, S)) == []
    assert same_bits(bdsp_model(blocks, S, "order"), C) == (m < 3)
    assert same_bits(bdsp_model(blocks, S, "fma"), C) == (m < 2)


@pytest.mark.gpu
@pytest.mark.parametrize("m,nb", BD_SHAPES)
def test_block_diagonal_times_sparse_and_lu_solve_bits(mg, m, nb):
    """`BlockDiagonal @ S`: the bits of bdsp_model with the blocks as given.  `.lu().solve(S)`: the bits of bdsp_model fed
    with getf2_inverse(block) -- the library multiplies by exactly the inverse it reports -- and, the blocks' condition
    numbers being below 100 (asserted by the CPU test of this case), np.linalg.solve to 1e-12 of the largest entry"""
    blocks, S, C = bd_case(m, nb)
    bd = mg.BlockDiagonal(blocks)
    dS = upload(mg, S)
    assert same_bits(download(bd @ dS), C)
    got = download(bd.lu().solve(dS))
    assert same_bits(got, bdsp_model(inverses(blocks), S))
    ref = np.linalg.solve(bd.todense(), S.scipy().toarray())
    assert np.abs(got.scipy().toarray() - ref).max() < 1e-12 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------
# 4. batched LU with real pivoting
# ------------------------------------------------------------------------------------------
LU_SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 33, 64]     # 1 .. 8: block_invert_kernel<M>; above: block_invert_any_kernel
LU_NB = 600                                                # three workgroups of one thread per block, the last partial
FAMILIES = ("reversed", "last_row", "ties", "perm_pow2", "dominant")


def _dominant(rng, m):
    """strictly diagonally dominant by rows AND by columns (2m on the diagonal, the rest in [-1, 1]) -- elimination keeps
    both, so the diagonal entry is the strict maximum of its column at every step: no exchange, no tie"""
    return rng.uniform(-1.0, 1.0, (m, m)) + 2.0 * m * np.diag(rng.choice([-1.0, 1.0], m))


def _tie_block(rng, m):
    """block upper triangular, diagonal blocks of 3 rows (then 2, then 1 for what is left): below the diagonal blocks
    all is zero, so a row is first modified at the step that opens its diagonal block.  There, column k of a 3-block
    reads (1, 4, -4): rows k + 1 and k + 2 tie and the FIRST, k + 1, has to be taken (a search with >= takes k + 2);
    a 2-block reads (4, -4): rows k and k + 1 tie, no exchange"""
    a = np.triu(rng.uniform(-1.0, 1.0, (m, m)))
    starts = []
    k = 0
    while k < m:
        size = min(3, m - k)
        a[k:k + size, k:k + size] = rng.uniform(8.0, 9.0, (size, size)) * rng.choice([-1.0, 1.0], (size, size))
        if size == 3:
            a[k:k + 3, k] = [1.0, 4.0, -4.0]
        elif size == 2:
            a[k:k + 2, k] = [4.0, -4.0]
        if size > 1:
            starts.append(k)
        k += size
    return a, starts


def lu_block(family, m, rng):
    """-> (block, expected piv, expected tie steps)"""
    ident = list(range(m))
    if family == "dominant":
        return _dominant(rng, m), ident, []
    if family == "reversed":      # row i holds row m - 1 - i of a dominant matrix: step k < m // 2 exchanges rows k and m - 1 - k, which
        piv = [m - 1 - k if k < m // 2 else k for k in range(m)]                     # puts both in place
        return _dominant(rng, m)[::-1].copy(), piv, []
    if family == "last_row":      # rows rotated up by one: the row wanted at step k always sits in the LAST row: an
        return np.roll(_dominant(rng, m), -1, axis=0), [m - 1] * m, []               # exchange at every step k < m - 1
    if family == "ties":          # (which row the steps inside a diagonal block take depends on the values: no claim)
        a, starts = _tie_block(rng, m)
        return a, None, starts
    if family == "perm_pow2":     # a cyclic shift composed with random transpositions, entries +-2^e
        perm = np.roll(np.arange(m), 1)
        for _ in range(m // 3):
            i, j = rng.integers(0, m, 2)
            perm[[i, j]] = perm[[j, i]]
        a = np.zeros((m, m))
        a[np.arange(m), perm] = rng.choice([-1.0, 1.0], m) * 2.0 ** rng.integers(-20, 21, m)
        return a, None, []
    raise KeyError(family)


@functools.lru_cache(maxsize=None)
def lu_case(m):
    """the distinct blocks of size m: every family, two draws of each up to m = 16 (one above: the reference is a Python
    loop), and their getf2 inverses; block b of the LU_NB device blocks is distinct block b mod their number"""
    rng = np.random.default_rng(2000 + m)
    fam, blocks, claims = [], [], []
    for draw in range(2 if m <= 16 else 1):
        for f in FAMILIES:
            a, piv, ties = lu_block(f, m, rng)
            fam.append(f), blocks.append(a), claims.append((piv, ties))
    blocks = np.stack(blocks)
    return fam, blocks, claims, inverses(blocks)


def tiled(distinct, nb):
    return distinct[np.arange(nb) % len(distinct)]


def sparse_with_diagonal_blocks(blocks, rng, per_col=2):
    """N x N CSC matrix whose diagonal blocks are `blocks` (their zeros not stored) plus random coupling outside them --
    far from block tridiagonal"""
    nb, m, _ = blocks.shape
    N = nb * m
    k, i, j = np.meshgrid(np.arange(nb), np.arange(m), np.arange(m), indexing="ij")
    rows, cols, vals = (k * m + i).ravel(), (k * m + j).ravel(), blocks.ravel()
    keep = vals != 0.0
    cc = np.repeat(np.arange(N), per_col)
    rr = rng.integers(0, N, cc.size)
    off = rr // m != cc // m
    A = sp.coo_matrix((np.concatenate((vals[keep], rng.uniform(-1.0, 1.0, int(off.sum())))),
                       (np.concatenate((rows[keep], rr[off])), np.concatenate((cols[keep], cc[off])))), shape=(N, N)).tocsc()
    A.sort_indices()
    return A


def block_inds(m, nb):
    """mBlockInds of contiguous aligned blocks: (m x nb), 1-based"""
    return np.arange(nb)[None, :] * m + np.arange(1, m + 1)[:, None]


@pytest.mark.parametrize("m", LU_SIZES)
def test_lu_families_pivot_as_claimed(m):
    """no GPU: the restatement's piv and tie record on every distinct block -- the exchanging families really exchange
    rows at the steps claimed, the ties are there and are resolved towards the first row, the dominant family never
    exchanges; the scaled permutations invert exactly; every restatement inverse is an inverse (LAPACK, sanity only)"""
    fam, blocks, claims, invs = lu_case(m)
    for f, a, (piv_claim, ties_claim), inv in zip(fam, blocks, claims, invs):
        _, piv, ties = getf2_factor(a)
        assert ties == ties_claim, (f, ties)
        if piv_claim is not None:
            assert piv == piv_claim, (f, piv)
        if f == "last_row":
            assert all(piv[k] != k for k in range(m - 1))
        if f == "reversed":
            assert sum(piv[k] != k for k in range(m)) == m // 2
        if f == "ties":
            for k in ties:                 # both tying rows are candidates; the one taken is the first of them
                col = np.abs(getf2_partial(a, k)[k:, k])
                first = k + int(np.nonzero(col == col.max())[0][0])
                assert piv[k] == first and np.count_nonzero(col == col.max()) == 2
            assert m < 2 or ties == list(range(0, m - 1, 3))
            assert m < 3 or any(piv[k] == k + 1 for k in ties)
        if f == "perm_pow2":
            assert m < 2 or any(piv[k] != k for k in range(m))
            exact = np.zeros((m, m))
            r, c = np.nonzero(a)
            exact[c, r] = 1.0 / a[r, c]
            assert np.array_equal(inv, exact)
        assert np.allclose(inv, np.linalg.inv(a), rtol=1e-9, atol=1e-12 * np.abs(inv).max())


def getf2_partial(a, steps):
    """the working array of the restatement after `steps` elimination steps (to look at the column a step chooses from)"""
    return getf2_factor(a, steps)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("m", LU_SIZES)
def test_batched_lu_with_pivoting_bits(mg, m):
    """600 blocks (three workgroups) of every family through both entries of K6, each inverse with == 0.0 difference from
    the restatement: BlockDiagonal(blocks).lu() -- column-major blocks, inverses read from the factorisation's device
    handle -- and BlockJacobi on a sparse matrix with these diagonal blocks -- row-major: up to m = 9 the blocks come from
    the block-tridiagonal scatter, above from the generic extraction (binary search)"""
    from agglomerationmultigrid1d_amd.api import _download_blocks
    fam, distinct, _, invs = lu_case(m)
    blocks, want = tiled(distinct, LU_NB), tiled(invs, LU_NB)
    lu = mg.BlockDiagonal(blocks).lu()
    got = _download_blocks(mg.default_context(), lu._dev.handle, LU_NB, m)
    bad = np.nonzero(np.abs(got - want).reshape(LU_NB, -1).max(axis=1) != 0.0)[0]
    assert bad.size == 0, ("column-major entry", [fam[b % len(fam)] for b in bad[:5]], bad[:5])
    A = sparse_with_diagonal_blocks(blocks, np.random.default_rng(m))
    S = mg.BlockJacobi(mg.DeviceOperator(A), block_inds(m, LU_NB))
    got = S.inverse_blocks()
    bad = np.nonzero(np.abs(got - want).reshape(LU_NB, -1).max(axis=1) != 0.0)[0]
    assert bad.size == 0, ("row-major entry", [fam[b % len(fam)] for b in bad[:5]], bad[:5])


def singular_structural(rng, m, k0):
    """rows of an upper triangular matrix with U[k0, k0] = 0, in random order: every step exchanges rows and eliminates
    nothing but zeros (exactly), and at step k0 the whole column is zero"""
    u = np.triu(rng.uniform(1.0, 2.0, (m, m)) * rng.choice([-1.0, 1.0], (m, m)))
    u[k0, k0] = 0.0
    return u[rng.permutation(m)].copy()


def singular_proportional(rng, m):
    """small integers, two rows in proportion 1 : 2 (a power of two: the rows stay in exact proportion through every
    elimination step that uses another pivot row); the zero pivot shows up after genuine eliminations, late"""
    for _ in range(200):
        a = rng.integers(-4, 5, (m, m)).astype(np.float64) + 6.0 * np.eye(m)
        i, j = rng.choice(m, size=2, replace=False)
        a[j] = 2.0 * a[i]
        try:
            getf2_factor(a)
        except SingularAtStep as e:
            if e.step > 0 and np.linalg.matrix_rank(np.delete(a, j, axis=0)) == m - 1:
                return a
    raise AssertionError("no draw became singular in floating point")


def singular_step(a):
    with pytest.raises(SingularAtStep) as e:
        getf2_factor(a)
    return e.value.step


@functools.lru_cache(maxsize=None)
def singular_case(m):
    rng = np.random.default_rng(3000 + m)
    good = np.stack([_dominant(rng, m) for _ in range(7)])
    return good, [singular_structural(rng, m, m - 1), singular_structural(rng, m, m // 2), singular_proportional(rng, m)]


@pytest.mark.parametrize("m", [3, 8, 12, 33])
def test_singular_blocks_are_singular_at_a_late_step(m):
    """no GPU: the restatement meets the zero pivot at the step claimed, k > 0 -- the first column does not give it away"""
    _, sing = singular_case(m)
    assert singular_step(sing[0]) == m - 1 and singular_step(sing[1]) == m // 2 and singular_step(sing[2]) > 0
    for a in sing:
        assert np.all(np.abs(a[:, 0]).max() > 0.0)


def both_entries_raise(mg, blocks, number):
    m, nb = blocks.shape[1], blocks.shape[0]
    with pytest.raises(mg.SingularException, match=rf"singular block {number} \("):
        mg.BlockDiagonal(blocks).lu()
    A = sparse_with_diagonal_blocks(blocks, np.random.default_rng(7))
    with pytest.raises(mg.SingularException, match=rf"singular block {number} \("):
        mg.BlockJacobi(mg.DeviceOperator(A), block_inds(m, nb))


@pytest.mark.gpu
@pytest.mark.parametrize("m", [3, 8, 12, 33])
def test_singular_block_reporting(mg, m):
    """SingularException with the 1-based number of the FIRST singular block, through both entries: blocks 517 and 301 of
    600 (workgroups 2 and 1: the order in which their atomicMin arrive is not fixed) -> 301; the very last block
    -> 600; every kind of late singularity on its own; and the entries work again afterwards"""
    good, sing = singular_case(m)
    blocks = tiled(good, LU_NB).copy()
    blocks[516], blocks[300] = sing[0], sing[2]
    both_entries_raise(mg, blocks, 301)
    blocks = tiled(good, LU_NB).copy()
    blocks[LU_NB - 1] = sing[1]
    both_entries_raise(mg, blocks, LU_NB)
    for k, a in enumerate(sing):
        blocks = tiled(good, 5).copy()
        blocks[k + 1] = a
        both_entries_raise(mg, blocks, k + 2)
    from agglomerationmultigrid1d_amd.api import _download_blocks
    lu = mg.BlockDiagonal(good).lu()      # held in a name: the factorisation frees its device handle when it is collected
    got = _download_blocks(mg.default_context(), lu._dev.handle, len(good), m)
    assert np.abs(got - inverses(good)).max() == 0.0


# ------------------------------------------------------------------------------------------
# 5. block extraction on arbitrary index lists
# ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extraction_matrix():
    """400 x 400 symmetric, about 6 entries per row, diagonal +-(6 .. 9) against off-diagonal entries in [-1, 1]"""
    rng = np.random.default_rng(140)
    N = 400
    r, c = rng.integers(0, N, 1000), rng.integers(0, N, 1000)
    keep = r != c
    R = sp.coo_matrix((rng.uniform(-1.0, 1.0, int(keep.sum())), (r[keep], c[keep])), shape=(N, N)).tocsr()
    A = sp.csc_matrix(R + R.T + sp.diags(rng.uniform(6.0, 9.0, N) * rng.choice([-1.0, 1.0], N)))
    A.sort_indices()
    return A


@functools.lru_cache(maxsize=None)
def extraction_case(m):
    """300 lists of m distinct indices: half grown from a row's stored neighbours (pairs that ARE stored), half random
    (pairs that mostly are not); shuffled inside a list, in no order across lists, overlapping; list 0 starts with N - 1
    and ends with 0"""
    rng = np.random.default_rng(141 + m)
    A = extraction_matrix()
    N = A.shape[0]
    lists = []
    for k in range(300):
        if k % 2:
            seed = int(rng.integers(0, N))
            near = [int(r) for r in A.indices[A.indptr[seed]:A.indptr[seed + 1]]][:m]
            rest = [int(r) for r in rng.permutation(N) if r not in near][:m - len(near)]
            idx = np.array(near + rest)
        else:
            idx = rng.choice(N, size=m, replace=False)
        lists.append(rng.permutation(idx))
    lists[0] = np.concatenate(([N - 1], [i for i in lists[0] if i not in (0, N - 1)][:m - 2], [0]))
    inds = np.stack(lists, axis=1)                                  # (m x nb), 0-based
    dense = A.toarray()
    blocks = np.stack([dense[np.ix_(idx, idx)] for idx in inds.T])
    return A, inds, blocks, inverses(blocks)


@pytest.mark.parametrize("m", [3, 7, 12])
def test_extraction_lists_are_unstructured(m):
    """no GPU: the lists are what the docstring of extraction_case says, and every block is well conditioned"""
    A, inds, blocks, _ = extraction_case(m)
    N = A.shape[0]
    assert np.abs(A - A.T).max() == 0.0 and np.all(A.diagonal() != 0.0) and 5.0 < A.nnz / N < 7.0
    assert inds.shape == (m, 300) and inds.size != N
    assert all(len(set(col)) == m for col in inds.T)
    assert inds[0, 0] == N - 1 and inds[-1, 0] == 0
    assert np.count_nonzero(np.any(np.diff(inds, axis=0) < 0, axis=0)) > 200         # not ascending inside a list
    assert np.count_nonzero(np.diff(inds.min(axis=0)) < 0) > 100                     # no order across lists
    assert np.bincount(inds.ravel(), minlength=N).max() >= 2                         # overlapping
    offdiag = blocks[:, ~np.eye(m, dtype=bool)]
    assert np.count_nonzero(offdiag) > 300 and np.count_nonzero(offdiag == 0.0) > 300   # stored and absent pairs
    assert max(np.linalg.cond(b) for b in blocks) < 1e6


@pytest.mark.gpu
@pytest.mark.parametrize("m", [3, 7, 12])
def test_block_extraction_on_arbitrary_lists_bits(mg, m):
    """AdditiveSchwarzSmoother on overlapping, unsorted lists: block k of inverse_blocks() is getf2_inverse(A[idx, idx]) to
    the bit -- read before any sweep (the first sweep reorders the blocks)"""
    A, inds, _, want = extraction_case(m)
    S = mg.AdditiveSchwarzSmoother(mg.DeviceOperator(A), inds + 1)
    got = S.inverse_blocks()
    bad = np.nonzero(np.abs(got - want).reshape(len(want), -1).max(axis=1) != 0.0)[0]
    assert bad.size == 0, bad[:10]


# ------------------------------------------------------------------------------------------
# 6. upload validation
# ------------------------------------------------------------------------------------------
# Read before run (setup_csc_upload, aggmg_csc_upload, DeviceOperator.__init__): the host entry takes nnz = colptr[n] - base
# and copies nnz entries of rowval / nzval -- so DeviceOperator refuses a colptr[n] that is negative or larger than the
# arrays BEFORE the library sees them (the C entry refuses a negative one itself; only the caller knows the lengths).
# csc_convert_colptr_kernel reads colptr64[j - 1], colptr64[j] and writes colptr[j] for j <= n only; the row pass is
# launched only once colptr is known to ascend from 0 to nnz, walks p in [0, nnz) and writes rowval[p] there, whatever
# the row index read.  No refusing path indexes anything with a value taken from the arrays.
def valid_matrix():
    return Csc.from_columns((5, 4), [([0, 2], [1.0, 2.0]), ([1], [3.0]), ([], []), ([0, 3, 4], [4.0, 5.0, 6.0])])


def raw_upload(mg, m, n, colptr, rowval, nzval, one_based):
    return mg.DeviceOperator((m, n, np.asarray(colptr, dtype=np.int64), np.asarray(rowval, dtype=np.int64),
                              np.asarray(nzval, dtype=np.float64), one_based))


def context_still_works(mg, one_based):
    V = valid_matrix()
    W = Csc.from_columns((4, 2), [([0, 1, 3], [1.0, -1.0, 0.5]), ([2], [2.0])])
    assert same_bits(download(upload(mg, V, one_based=one_based).matmul(upload(mg, W, one_based=one_based))), spmm_model(V, W))


MALFORMED = {
    # name: (colptr, rowval of the 5 x 4 matrix, 0-based; exception; message)
    "colptr_decreasing": ([0, 2, 1, 3, 6], [0, 2, 1, 0, 3, 4], "ArgumentError", "colptr not monotone"),
    "colptr_first_not_base": ([1, 2, 3, 3, 6], [0, 2, 1, 0, 3, 4], "ArgumentError", "colptr does not start at the index base"),
    "colptr_inner_beyond_end": ([0, 2, 7, 7, 6], [0, 2, 1, 0, 3, 4], "ArgumentError", "colptr not monotone"),
    "colptr_end_beyond_arrays": ([0, 2, 3, 3, 9], [0, 2, 1, 0, 3, 4], "ArgumentError", "colptr ends at 9 entries"),
    "colptr_end_negative": ([0, 0, 0, 0, -3], [0, 2, 1, 0, 3, 4], "ArgumentError", "colptr ends at -3 entries"),
    "row_equal_m": ([0, 2, 3, 3, 6], [0, 2, 1, 0, 3, 5], "DimensionMismatch", "row index out of range"),
    "row_below_base": ([0, 2, 3, 3, 6], [-1, 2, 1, 0, 3, 4], "DimensionMismatch", "row index out of range"),
    "rows_equal": ([0, 2, 3, 3, 6], [0, 2, 1, 0, 3, 3], "ArgumentError", "row indices not strictly ascending"),
    "rows_descending": ([0, 2, 3, 3, 6], [2, 0, 1, 0, 3, 4], "ArgumentError", "row indices not strictly ascending"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("one_based", [0, 1])
@pytest.mark.parametrize("name", list(MALFORMED))
def test_upload_refuses_malformed_csc(mg, name, one_based):
    colptr, rowval, exc, msg = MALFORMED[name]
    colptr, rowval = np.array(colptr) + one_based, np.array(rowval) + one_based
    with pytest.raises(getattr(mg, exc), match=msg):
        raw_upload(mg, 5, 4, colptr, rowval, np.arange(1.0, 7.0), one_based)
    context_still_works(mg, one_based)


@pytest.mark.gpu
def test_upload_entry_guards_of_the_c_abi(mg):
    """the C entry itself: a negative entry count and a colptr of the wrong length never reach a copy"""
    ctx = mg.default_context()
    colptr = np.array([0, 0, 0, 0, -3], dtype=np.int64)
    rowval, nzval = np.zeros(6, dtype=np.int64), np.zeros(6)
    h = ctypes.c_void_p()
    st = ctx.lib.aggmg_csc_upload(ctx.handle, 5, 4, colptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  rowval.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  nzval.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 0, 0, ctypes.byref(h))
    with pytest.raises(mg.ArgumentError, match="inconsistent colptr"):
        ctx.check(st)
    assert not h.value
    with pytest.raises(mg.ArgumentError, match="colptr must hold n \\+ 1 = 5 entries"):
        raw_upload(mg, 5, 4, [0, 2, 3, 6], [0, 2, 1, 0, 3, 4], np.arange(1.0, 7.0), 0)
    context_still_works(mg, 0)


def _edge_cases():
    rng = np.random.default_rng(150)
    return {"zero_entries": Csc.from_columns((6, 5), [([], [])] * 5),
            "zero_columns": Csc.from_columns((6, 0), []),
            "one_column": Csc.from_columns((6, 1), [([0, 5], [-0.0, 2.5])]),
            "257_columns": random_csc(rng, 9, 257, lo=0, hi=4)}


@pytest.mark.gpu
@pytest.mark.parametrize("one_based", [0, 1])
@pytest.mark.parametrize("name", ["zero_entries", "zero_columns", "one_column", "257_columns"])
def test_upload_round_trip_of_well_formed_edge_cases(mg, name, one_based):
    """to_scipy() returns the uploaded arrays bit for bit (stored zeros, -0.0 included); rowval / nzval longer than colptr
    uses -- a SparseMatrixCSC may carry such a tail -- are read up to colptr[n] only"""
    T = _edge_cases()[name]
    op = upload(mg, T, one_based=one_based)
    assert op.shape == T.shape and op.nnz == T.nnz and same_bits(download(op), T)
    tail = raw_upload(mg, T.shape[0], T.shape[1], T.indptr + one_based, np.concatenate((T.indices + one_based, [10 ** 6, -7])),
                      np.concatenate((T.data, [np.nan, 1.0])), one_based)
    assert tail.nnz == T.nnz and same_bits(download(tail), T)
