"""The generic CSR kernels (csr_stream_kernel, csr_row_kernel<64>, csr_rowthread_kernel, csr_rowthread_band_kernel) on
unstructured sparsity patterns: long rows, empty rows, row blocks at their caps, wide rows, 1 x 1 ... 2 x 2 operators, an
algebraic three-level hierarchy, and the A/B switches of launch_csr in child processes.

Every result is held, ROW BY ROW, to a running-error bound around an exact (rational) reference -- see `row_bound` --
and, where the kernels' comments fix the arithmetic (products rounded, then added one at a time in ascending stored
column order), to the bits of a float64 loop that does exactly that.  The helpers are tested without a GPU
(test_reference_model_and_bound_on_every_pattern): the float64 model lies inside the bound on every row of every
pattern, and two deliberately wrong models (last entry of a row dropped, first entry of the next row added) are rejected
on every row they touch.

Which kernel a pattern reaches is decided by launch_csr / setup_stream_blocks from the pattern's mean and longest row
and from its bandwidth; every pattern asserts these from its own arrays against the constants read out of the sources
(`source_constants`), so that a retuned constant fails here instead of silently moving a pattern to another kernel."""
import functools
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "agglomerationmultigrid1d_amd", "csrc")

U = Fraction(1, 2 ** 53)          # unit roundoff of float64, round to nearest
ALPHA = 2.0 / 3.0
MODES = ("set", "add", "residual", "jacobi")


@pytest.fixture(scope="module")
def mg():
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    return mg


# ------------------------------------------------------------------------------------------
# the constants the patterns were built for, read out of the sources
# ------------------------------------------------------------------------------------------
BUILT_FOR = {"stream_nnz": 1536, "stream_rows": 256, "threads": 256, "rowthread_max": 32, "mean_switch": 48.0,
             "band_max_bw": 32}


def source_constants():
    """kStreamNnz (AGGMG_STREAM_NNZ), kStreamRows, kThreads, kRowThreadMax, kBandMaxBw and the mean row length above which
    setup_stream_blocks leaves an operator to csr_row_kernel, as the sources state them"""
    text = ""
    for name in ("kernels.hpp", "setup.hip", "internal.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            text += f.read() + "\n"

    def find(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, f"expected exactly one match of {pattern!r} in the kernel sources, found {len(m)}"
        return m[0]

    threads = int(find(r"constexpr\s+int\s+kThreads\s*=\s*(\d+)\s*;"))
    rows = find(r"#define\s+AGGMG_STREAM_ROWS\s+(\w+)")
    return {"stream_nnz": int(find(r"#define\s+AGGMG_STREAM_NNZ\s+(\d+)")),
            "stream_rows": threads if rows == "kThreads" else int(rows),
            "threads": threads,
            "rowthread_max": int(find(r"constexpr\s+int\s+kRowThreadMax\s*=\s*(\d+)\s*;")),
            "mean_switch": float(find(r"\(double\)d->nnz\s*/\s*\(double\)d->nrows\s*>\s*([0-9.]+)\s*\)\s*return\s+AGGMG_OK")),
            "band_max_bw": int(find(r"constexpr\s+int\s+kBandMaxBw\s*=\s*(\d+)\s*;"))}


def stream_blocks(indptr, max_nnz, max_rows):
    """the row blocks csr_stream_kernel is launched on, by the rule stated above stream_row_blocks (host_plan.hpp): runs of
    consecutive rows of at most max_nnz entries and max_rows rows, a longer row alone"""
    n = len(indptr) - 1
    blk, r = [0], 0
    while r < n:
        e = r + 1
        while e < n and e - r < max_rows and indptr[e + 1] - indptr[r] <= max_nnz:
            e += 1
        blk.append(e)
        r = e
    return np.array(blk)


def bandwidth(M):
    coo = M.tocoo()
    return int(np.abs(coo.row - coo.col).max()) if coo.nnz else 0


# ------------------------------------------------------------------------------------------
# patterns
# ------------------------------------------------------------------------------------------
def _magnitudes(rng, n, lo, hi):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(lo, hi, n)


def _vector(rng, n):
    """entries of either sign in [0.5, 2): none so small that a wrong product with it could hide"""
    return rng.choice([-1.0, 1.0], n) * rng.uniform(0.5, 2.0, n)


def assemble(rng, shape, row_cols, zeros=True):
    """CSR matrix with the given (ascending, distinct) columns per row.  Values: either sign, magnitudes spread over
    1e-6 .. 1e6, some stored zeros -- but the first and the last entry of a row are never zero and at least 1e3 in size (a
    kernel that loses the end of a row or reads on into the next one is then off by far more than the bound), and the
    diagonal of a square matrix lies in 1 .. 1e3 (point Jacobi divides by it)."""
    nrows, ncols = shape
    lens = np.array([len(c) for c in row_cols], dtype=np.int64)
    indptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    indices = (np.concatenate(row_cols) if lens.sum() else np.zeros(0)).astype(np.int32)
    nnz = int(lens.sum())
    data = _magnitudes(rng, nnz, -6.0, 6.0)
    if zeros:
        data[rng.random(nnz) < 0.04] = 0.0
    ends = np.unique(np.concatenate((indptr[:-1][lens > 0], indptr[1:][lens > 0] - 1))).astype(np.int64)
    data[ends] = _magnitudes(rng, ends.size, 3.0, 6.0)
    if nrows == ncols:
        rows = np.repeat(np.arange(nrows), lens)
        on = np.nonzero(rows == indices)[0]
        data[on] = _magnitudes(rng, on.size, 0.0, 3.0)
    M = sp.csr_matrix((data, indices, indptr), shape=shape)
    assert M.has_sorted_indices and M.nnz == nnz
    return M


def _random_cols(rng, ncols, k, must=None, allowed=None):
    pool = np.arange(ncols) if allowed is None else allowed
    c = rng.choice(pool, size=k, replace=False)
    if must is not None and must not in c:
        c[0] = must
    return np.sort(c)


def _long_rows(rng, ends):
    N = 2000
    rows = [_random_cols(rng, N, 5, must=i) for i in range(N)]
    if ends:    # the workgroup-reduced rows first and last
        special = {0: 2000, 1: 1536, N - 3: 1535, N - 2: 1, N - 1: 1537}
    else:
        special = {300: 1537, 777: 1536, 1200: 1535, 1201: 1, 1650: 2000}
    for i, k in special.items():
        rows[i] = _random_cols(rng, N, k, must=i)
    return assemble(rng, (N, N), rows)


def _empty_runs(n):
    """runs of empty rows at the start, in the middle and at the end of n rows; the long one (300 rows) covers a whole
    256-row block"""
    empty = np.zeros(n, dtype=bool)
    empty[:10] = True
    empty[100:105] = True
    empty[500:800] = True
    empty[n - 10:] = True
    return empty


def _empty_rows_transfer(rng):
    m, n = 1500, 900
    empty_r, empty_c = _empty_runs(m), _empty_runs(n)
    allowed = np.nonzero(~empty_c)[0]
    rows = [np.zeros(0, dtype=np.int64) if empty_r[i] else _random_cols(rng, n, int(rng.integers(1, 6)), allowed=allowed)
            for i in range(m)]
    return assemble(rng, (m, n), rows)


def _empty_rows_transposed(rng):
    """the transposed pattern (900 x 1500: its empty rows are the transfer's empty columns), values of its own so that
    the ends of ITS rows are the large entries"""
    P = sp.csr_matrix(_empty_rows_transfer(rng).T)
    P.sort_indices()
    return assemble(rng, P.shape, [P.indices[P.indptr[i]:P.indptr[i + 1]] for i in range(P.shape[0])])


def _empty_rows_square(rng):
    N = 1500
    empty = _empty_runs(N)
    rows = [np.array([i]) if empty[i] else _random_cols(rng, N, int(rng.integers(2, 6)), must=i) for i in range(N)]
    return assemble(rng, (N, N), rows)


def _caps(rng, ones):
    """`ones` rows holding the diagonal alone, 256 rows of exactly 6 entries, 500 rows of 7"""
    N = ones + 256 + 500
    rows = [np.array([i]) for i in range(ones)]
    rows += [_random_cols(rng, N, 6, must=i) for i in range(ones, ones + 256)]
    rows += [_random_cols(rng, N, 7, must=i) for i in range(ones + 256, N)]
    return assemble(rng, (N, N), rows)


def _wide_lengths(rng, n, hi):
    lens = rng.integers(60, hi + 1, n)
    lens[lens % 64 == 0] += 1
    return lens


def _wide_square(rng):
    N = 301
    lens = _wide_lengths(rng, N, 130)
    lens[150] = 1
    return assemble(rng, (N, N), [_random_cols(rng, N, int(k), must=i) for i, k in enumerate(lens)])


def _wide_rect(rng):
    m, n = 301, 203
    lens = _wide_lengths(rng, m, 130)
    lens[17] = 1
    lens[222] = 0
    return assemble(rng, (m, n), [_random_cols(rng, n, int(k)) for k in lens])


def _tiny(rng, shape):
    m, n = shape
    return assemble(rng, shape, [np.arange(n) for _ in range(m)], zeros=False)


# name -> (builder, seed, kernel the pattern is meant for)
PATTERNS = {
    "long_rows_interior": (lambda g: _long_rows(g, False), 11, "stream"),
    "long_rows_ends": (lambda g: _long_rows(g, True), 12, "stream"),
    "empty_rows": (_empty_rows_transfer, 13, "stream"),
    "empty_rows_transposed": (_empty_rows_transposed, 13, "stream"),
    "empty_rows_square": (_empty_rows_square, 14, "stream"),
    "caps": (lambda g: _caps(g, 600), 15, "stream"),
    "caps_aligned": (lambda g: _caps(g, 768), 16, "stream"),
    "wide_rows_square": (_wide_square, 17, "row64"),
    "wide_rows_rect": (_wide_rect, 18, "row64"),
    "tiny_1x1": (lambda g: _tiny(g, (1, 1)), 19, "stream"),
    "tiny_1x7": (lambda g: _tiny(g, (1, 7)), 20, "stream"),
    "tiny_7x1": (lambda g: _tiny(g, (7, 1)), 21, "stream"),
    "tiny_2x2": (lambda g: _tiny(g, (2, 2)), 22, "stream"),
}


class Case:
    """one pattern with its vectors, the exact row sums s_i and S_i = sum |a_ij| |x_j| (Fractions), and its row lengths"""

    def __init__(self, name, M=None, seed=None):
        if M is None:
            build, seed, self.kernel = PATTERNS[name]
            M = build(np.random.default_rng(seed))
        self.name = name
        M = sp.csr_matrix(M)
        M.sort_indices()
        self.M = M
        self.indptr, self.indices, self.data = M.indptr, M.indices, M.data
        self.lens = np.diff(M.indptr)
        m, n = M.shape
        self.square = m == n
        rng = np.random.default_rng(1000 + seed)
        self.x = _vector(rng, n)
        self.y0 = _vector(rng, m)
        self.b = _vector(rng, m)
        self.diag = M.diagonal() if self.square else None
        self.modes = MODES if self.square and np.all(self.diag != 0.0) else MODES[:2]
        self.s, self.S = exact_row_sums(self.indptr, self.indices, self.data, self.x)

    @property
    def mean_row(self):
        return self.M.nnz / self.M.shape[0]


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ------------------------------------------------------------------------------------------
# exact reference, bound, float64 model
# ------------------------------------------------------------------------------------------
def exact_row_sums(indptr, indices, data, x):
    """s_i = sum_j a_ij x_j and S_i = sum_j |a_ij| |x_j| over the stored entries, exactly (every float64 is a rational)"""
    fx = [Fraction(float(v)) for v in x]
    s, S = [], []
    for i in range(len(indptr) - 1):
        t, T = Fraction(0), Fraction(0)
        for p in range(indptr[i], indptr[i + 1]):
            prod = Fraction(float(data[p])) * fx[indices[p]]
            t += prod
            T += abs(prod)
        s.append(t)
        S.append(T)
    return s, S


def gamma(n):
    return n * U / (1 - n * U)


def row_bound(mode, n, S, y=0, b=0, x=0, scale=0):
    """Bound on |computed - exact| for one row of n stored entries, u = 2^-53, gamma_k = k u / (1 - k u).

    Every floating-point operation returns its exact result times (1 + d), |d| <= u (no overflow or underflow at these
    magnitudes; an FMA is one such operation where separate multiply and add are two).  In a computed sum of n products a
    product passes through its own rounding and through at most n - 1 additions, whatever the order of the additions -- one
    accumulator, several accumulators combined by a tree, partial sums of a wave or a workgroup -- and through fewer when
    products are fused into additions.  So the computed sum is  sum_j a_ij x_j (1 + t_j)  with |t_j| <= gamma_n  and

        y = A x        |got - s_i| <= gamma_n S_i,                              S_i = sum_j |a_ij| |x_j|.

    One more operation c -/+ sum multiplies every term, c included, by one more (1 + d):

        y += A x       |got - (y_i + s_i)| <= gamma_{n+1} (S_i + |y_i|)
        b - A x        |got - (b_i - s_i)| <= gamma_{n+1} (S_i + |b_i|).

    A point-Jacobi sweep x_i + alpha (b_i - s_i) / d_i adds a division, a multiplication by alpha and an addition to the
    residual: three more roundings on every term of b_i - sum, the last of them on x_i as well (contracting alpha * q into
    the addition only removes one of them):

        |got - exact| <= u |x_i| + |alpha / d_i| gamma_{n+4} (S_i + |b_i|)          (scale = |alpha / d_i|).

    A row without entries sums nothing: gamma_0 = 0, and the tests ask y = A x, y += A x and b - A x for exactly 0, y_i
    and b_i there.  Nothing measured enters the bound."""
    if mode == "set":
        return gamma(n) * S
    if mode == "add":
        return gamma(n + 1) * (S + abs(y))
    if mode == "residual":
        return gamma(n + 1) * (S + abs(b))
    return U * abs(x) + scale * gamma(n + 4) * (S + abs(b))


def exact_and_bound(c, mode, alpha=ALPHA):
    """per row: the exact result of `mode` on case c and the bound on a computed one"""
    ex, bd = [], []
    fa = Fraction(alpha)
    for i in range(c.M.shape[0]):
        n, s, S = int(c.lens[i]), c.s[i], c.S[i]
        if mode == "set":
            ex.append(s)
            bd.append(row_bound(mode, n, S))
        elif mode == "add":
            y = Fraction(float(c.y0[i]))
            ex.append(y + s)
            bd.append(row_bound(mode, n, S, y=y))
        elif mode == "residual":
            b = Fraction(float(c.b[i]))
            ex.append(b - s)
            bd.append(row_bound(mode, n, S, b=b))
        else:
            b, x, d = Fraction(float(c.b[i])), Fraction(float(c.x[i])), Fraction(float(c.diag[i]))
            ex.append(x + fa * (b - s) / d)
            bd.append(row_bound(mode, n, S, b=b, x=x, scale=abs(fa / d)))
    return ex, bd


def bad_rows(c, mode, got, alpha=ALPHA):
    """rows of `got` outside the bound around the exact result (every row is looked at; a row without entries has to be
    exact in y = A x, y += A x and b - A x)"""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == (c.M.shape[0],)
    if not np.all(np.isfinite(got)):
        return list(range(got.size))
    ex, bd = exact_and_bound(c, mode, alpha)
    bad = []
    for i in range(got.size):
        err = abs(Fraction(float(got[i])) - ex[i])
        limit = bd[i] if (c.lens[i] > 0 or mode == "jacobi") else 0
        if err > limit:
            bad.append(i)
    return bad


def model_sums(c, corrupt=None):
    """float64 restatement of the short-row arithmetic of csr_stream_kernel / csr_rowthread_kernel: every product rounded
    to double, the products of a row added one at a time, from 0.0, in ascending stored column order.
    corrupt='drop': the last entry of every row left out; 'extra': the entry stored after the row's last one added."""
    ip, ci, v, x = c.indptr, c.indices, c.data, c.x
    out = np.zeros(len(ip) - 1)
    for i in range(len(ip) - 1):
        p0, p1 = int(ip[i]), int(ip[i + 1])
        if corrupt == "drop":
            p1 = max(p0, p1 - 1)
        if corrupt == "extra" and p1 < len(v):
            p1 += 1
        acc = 0.0
        for p in range(p0, p1):
            acc = acc + float(v[p]) * float(x[ci[p]])
        out[i] = acc
    return out


def finish(c, mode, acc, alpha=ALPHA):
    """the kernels' last step on the row sums, one float64 operation at a time (no contraction)"""
    if mode == "set":
        return acc.copy()
    if mode == "add":
        return c.y0 + acc
    if mode == "residual":
        return c.b - acc
    return c.x + alpha * ((c.b - acc) / c.diag)


def corrupted_term(c, mode, corrupt, alpha=ALPHA):
    """|what the corruption changes in the exact result| per row (0: the row is not affected)"""
    ip, ci, v = c.indptr, c.indices, c.data
    out = []
    for i in range(len(ip) - 1):
        p = int(ip[i + 1]) - 1 if corrupt == "drop" else int(ip[i + 1])
        if (corrupt == "drop" and c.lens[i] == 0) or p >= len(v):
            out.append(Fraction(0))
            continue
        t = abs(Fraction(float(v[p])) * Fraction(float(c.x[ci[p]])))
        if mode == "jacobi":
            t *= abs(Fraction(alpha) / Fraction(float(c.diag[i])))
        out.append(t)
    return out


def check_branch(c, k):
    """the pattern reaches the kernel and the branches it was built for (k: source_constants())"""
    assert k == BUILT_FOR
    blk = stream_blocks(c.indptr, k["stream_nnz"], k["stream_rows"])
    brows, bnnz = np.diff(blk), np.diff(c.indptr[blk])
    if c.kernel == "stream":
        assert c.mean_row <= k["mean_switch"]
    else:
        assert c.mean_row > k["mean_switch"]          # setup_stream_blocks: lanes-per-row kernel, 64 lanes
        assert c.M.shape[0] % (k["threads"] // 64) != 0   # a partial last workgroup
        assert np.all(c.lens[c.lens > 0] % 64 != 0) and 1 in c.lens and c.lens.max() > 64
        assert c.square or 0 in c.lens
    if c.name.startswith("long_rows"):
        assert c.lens.max() > k["stream_nnz"] and bandwidth(c.M) > k["band_max_bw"]
        for want in (k["stream_nnz"] + 1, k["stream_nnz"], k["stream_nnz"] - 1, c.M.shape[1]):
            assert want in c.lens
        i = int(np.nonzero(c.lens == k["stream_nnz"] - 1)[0][0])
        assert c.lens[i + 1] == 1 and i in blk and i + 2 in blk and i + 1 not in blk     # 1535 + 1 entries: one block
        lone = [int(r) for r in np.nonzero(c.lens > k["stream_nnz"])[0]]
        assert all(r in blk and r + 1 in blk for r in lone)                              # a long row stands alone
        if c.name.endswith("ends"):
            assert c.lens[0] > k["stream_nnz"] and c.lens[-1] > k["stream_nnz"]
    if c.name in ("empty_rows", "empty_rows_transposed"):
        assert c.lens[0] == 0 and c.lens[-1] == 0 and np.any((brows == k["stream_rows"]) & (bnnz == 0))
        assert np.any(np.diff(sp.csc_matrix(c.M).indptr) == 0)                           # empty columns too
    if c.name == "empty_rows_square":
        assert np.count_nonzero(c.lens == 1) >= 300 and bandwidth(c.M) > k["band_max_bw"]
    if c.name.startswith("caps"):
        assert bandwidth(c.M) > k["band_max_bw"]
        assert np.any((brows == k["stream_rows"]) & (bnnz == k["stream_rows"]))          # the row cap binds
        assert np.any((brows < k["stream_rows"]) & (bnnz > k["stream_nnz"] - 7))         # the entry cap binds
        assert np.any(bnnz == k["stream_nnz"])                                           # a block filled exactly
        assert brows[-1] < brows[-2]                                                     # ragged last block
    if c.name == "caps_aligned":
        assert np.any((brows == k["stream_rows"]) & (bnnz == k["stream_nnz"]))           # both caps at once
    if c.name.startswith("tiny"):
        assert len(blk) == 2


# ------------------------------------------------------------------------------------------
# CPU self-test of the helpers
# ------------------------------------------------------------------------------------------
def test_source_constants_are_the_ones_the_patterns_were_built_for():
    assert source_constants() == BUILT_FOR


@pytest.mark.parametrize("name", list(PATTERNS))
def test_reference_model_and_bound_on_every_pattern(name):
    """no GPU: the float64 sequential model passes the per-row check on every row and in every mode the pattern allows
    (the bound is not vacuous and the exact reference is consistent with it); the model with the last entry of each row
    dropped and the one with the entry after the row added are rejected on every row they touch, and on no other.  That
    the changed term exceeds the bound is asserted first: 4 x the bound, since the wrong model's own rounding (at most the
    bound of a row one entry longer, which also holds the extra term) must not bring it back inside."""
    c = case(name)
    check_branch(c, source_constants())
    for mode in c.modes:
        assert bad_rows(c, mode, finish(c, mode, model_sums(c))) == []
        _, bd = exact_and_bound(c, mode)
        for corrupt in ("drop", "extra"):
            term = corrupted_term(c, mode, corrupt)
            affected = [i for i, t in enumerate(term) if t != 0]
            if corrupt == "drop":
                assert affected == [i for i in range(len(term)) if c.lens[i] > 0]
            else:
                assert affected == [i for i in range(len(term)) if c.indptr[i + 1] < c.M.nnz]
            for i in affected:
                assert term[i] > 4 * bd[i], (mode, corrupt, i)
            assert bad_rows(c, mode, finish(c, mode, model_sums(c, corrupt))) == affected, (mode, corrupt)


# ------------------------------------------------------------------------------------------
# the kernels on the patterns
# ------------------------------------------------------------------------------------------
def device_modes(mg, c, alpha=ALPHA, sweeps=(2, 3)):
    """every mode case c allows through the device, by the Python mirror: y = M x as the restriction with M' uploaded
    (its CSC arrays are M's CSR), y += M x as the prolongation-add of M (row-gather CSR from setup_transpose), b - M x and
    point-Jacobi sweeps with M as a stiffness operator whose smoother keeps off the structured kernels."""
    from agglomerationmultigrid1d_amd import _lib
    out = {}
    Mt = mg.DeviceOperator(sp.csc_matrix(c.M.T), _lib.OP_TRANSFER)
    out["set"] = mg.restrict(Mt, c.x)
    Mo = mg.DeviceOperator(c.M, _lib.OP_TRANSFER)
    out["add"] = mg.prolong_add(Mo, c.x, c.y0)
    T = Mo.transpose().to_scipy()
    out["transpose"] = (T.indptr.copy(), T.indices.copy(), T.data.copy(), T.shape)
    if "residual" in c.modes:
        A = mg.DeviceOperator(c.M)
        out["residual"] = mg.residual(A, c.x, c.b)
        S = mg.JacobiSmoother(A, detect=False)
        assert not S.structured
        out["jacobi"] = mg.smooth(A, S, c.x, c.b, alpha, 1)
        for ns in sweeps:
            step = c.x
            for _ in range(ns):
                step = mg.smooth(A, S, step, c.b, alpha, 1)
            out[f"jacobi{ns}"] = mg.smooth(A, S, c.x, c.b, alpha, ns)
            out[f"jacobi{ns}_single"] = step
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PATTERNS))
def test_generic_csr_on_pattern(mg, name):
    """Every mode the pattern's shape allows: the per-row bound on EVERY row; on the rows of short-row stream blocks
    (operators with a mean row of at most 48 entries, rows of at most 1536) y = A x, y += A x and b - A x equal the
    sequential float64 model bit for bit; a point-Jacobi sweep ends in x + alpha * yy, which the compiler may contract into
    one FMA, so it gets the bound only.  csr_row_kernel<64> (mean row above 48) and the long-row branch add partial sums
    in another order: the bound only.  mg.smooth(..., ns) equals ns single sweeps bit for bit; the device transposition
    (setup_transpose) gives SciPy's row-major arrays of the matrix, stored zeros included, bit for bit."""
    c = case(name)
    k = source_constants()
    check_branch(c, k)
    got = device_modes(mg, c)
    model = model_sums(c)
    short = c.lens <= k["stream_nnz"]
    for mode in c.modes:
        assert bad_rows(c, mode, got[mode]) == [], mode
        if c.kernel == "stream" and mode != "jacobi":
            want = finish(c, mode, model)
            assert np.array_equal(got[mode][short], want[short]), (mode, np.nonzero((got[mode] != want) & short)[0][:10])
    if "jacobi" in c.modes:
        for ns in (2, 3):
            assert np.array_equal(got[f"jacobi{ns}"], got[f"jacobi{ns}_single"]), ns
    indptr, indices, data, shape = got["transpose"]
    assert shape == (c.M.shape[1], c.M.shape[0])
    assert np.array_equal(indptr, c.indptr) and np.array_equal(indices, c.indices) and np.array_equal(data, c.data)
    assert np.array_equal(np.signbit(data), np.signbit(c.data))


# ------------------------------------------------------------------------------------------
# a V-cycle through generic levels of an algebraic hierarchy
# ------------------------------------------------------------------------------------------
def algebraic_hierarchy(rng, n0=600):
    """A0: graph Laplacian + I of a random sparse graph under a random symmetric permutation; L_k: piecewise-constant
    aggregation, ragged aggregates of 2 .. 5 nodes; A_{k+1} = L_k' A_k L_k"""
    i = np.arange(n0)
    src = np.concatenate((i[:-1], rng.integers(0, n0, 2 * n0)))        # a path (connected) plus random edges
    dst = np.concatenate((i[1:], rng.integers(0, n0, 2 * n0)))
    keep = src != dst
    W = sp.coo_matrix((rng.uniform(0.5, 2.0, keep.sum()), (src[keep], dst[keep])), shape=(n0, n0)).tocsr()
    W = W + W.T
    A = sp.diags(np.asarray(W.sum(axis=1)).ravel()) - W + sp.identity(n0)
    perm = rng.permutation(n0)
    A = sp.csc_matrix(A[perm][:, perm])
    As, Ls = [A], []
    for _ in range(2):
        n = As[-1].shape[0]
        sizes = []
        while sum(sizes) < n:
            sizes.append(int(rng.choice([2, 3, 4, 5], p=[0.1, 0.2, 0.3, 0.4])))
        sizes[-1] -= sum(sizes) - n
        if sizes[-1] < 2:                       # a remainder of 0 or 1 joins the aggregate before it; 6 become 3 + 3
            last = sizes.pop()
            sizes[-1] += last
            if sizes[-1] > 5:
                sizes[-1:] = [3, sizes[-1] - 3]
        agg = np.repeat(np.arange(len(sizes)), sizes)
        L = sp.csc_matrix((np.ones(n), (rng.permutation(n), agg)), shape=(n, len(sizes)))
        Ls.append(L)
        As.append(sp.csc_matrix(L.T @ As[-1] @ L))
    return As, Ls


def dense_vcycle(As, Ls, x0, b, nPre, nPost, alpha, k=0):
    """src/solvers.jl:19-50 in dense NumPy, point-Jacobi smoothers, a dense solve on the coarsest level"""
    A = As[k].toarray()
    if k == len(As) - 1:
        return np.linalg.solve(A, b)
    d = As[k].diagonal()
    L = Ls[k].toarray()
    v = x0.copy()
    for _ in range(nPre):
        v = v + alpha * (b - A @ v) / d
    rc = L.T @ (b - A @ v)
    v = v + L @ dense_vcycle(As, Ls, np.zeros(len(rc)), rc, nPre, nPost, alpha, k + 1)
    for _ in range(nPost):
        v = v + alpha * (b - A @ v) / d
    return v


@pytest.mark.gpu
def test_vcycle_through_generic_levels_of_an_algebraic_hierarchy(mg):
    """three levels without any finite-element structure: neither banded nor an element chain, transfers with ragged
    aggregates -- both smoothed levels run the generic kernels (stream kernel: mean row <= 48, one sweep per launch:
    bandwidth > 32) and the coarsest, nearly dense operator goes to the direct solve; V(3,3), V(1,2), V(0,1) against the
    dense NumPy restatement at the project's V-cycle tolerance"""
    k = source_constants()
    rng = np.random.default_rng(31)
    As, Ls = algebraic_hierarchy(rng)
    assert As[0].shape[0] == 600 and As[2].shape[0] <= 40
    for A, L in zip(As[:2], Ls):
        assert bandwidth(A) > k["band_max_bw"] and A.nnz / A.shape[0] <= k["mean_switch"]
        sizes = np.diff(L.indptr)
        assert sizes.min() >= 2 and sizes.max() <= 5 and len(set(sizes)) == 4
    ops = [mg.DeviceOperator(A) for A in As]
    sms = [mg.JacobiSmoother(op, detect=False) for op in ops[:2]]
    H = mg.MeshHierarchy(None, ops, sms, Ls)
    assert H.level_kinds()[:-1] == ['generic', 'generic']
    N = As[0].shape[0]
    b, x0 = rng.standard_normal(N), rng.standard_normal(N)
    A0 = As[0].toarray()
    for nPre, nPost in ((3, 3), (1, 2), (0, 1)):
        x = mg.multigrid_v_cycle(H, x0, b, nPre=nPre, nPost=nPost)
        v = dense_vcycle(As, Ls, x0, b, nPre, nPost, ALPHA)
        assert np.linalg.norm(A0 @ (x - v)) <= 1e-12 * np.linalg.norm(b), (nPre, nPost)


# ------------------------------------------------------------------------------------------
# the A/B switches of launch_csr / setup_stream_blocks, one child process at a time
# ------------------------------------------------------------------------------------------
def _ab_short_rows(rng):
    """not banded, every row of at most 32 entries (csr_rowthread_kernel takes it), more than one workgroup of rows"""
    N = 700
    lens = rng.integers(1, 33, N)
    lens[5], lens[6] = 32, 1
    return assemble(rng, (N, N), [_random_cols(rng, N, int(k), must=i) for i, k in enumerate(lens)])


def _ab_banded(rng):
    """entries within 5 of the diagonal, ragged rows, diagonally dominant (so that sweeps stay bounded), two workgroups
    of rows with a halo between them"""
    N, bw = 300, 5
    rows = []
    for i in range(N):
        near = np.arange(max(0, i - bw), min(N, i + bw + 1))
        pick = near[(rng.random(near.size) < 0.6) | (near == i)]
        rows.append(pick)
    rows[0] = np.union1d(rows[0], [bw])
    rows[N - 1] = np.union1d(rows[N - 1], [N - 1 - bw])          # the band's edge is really there
    M = assemble(rng, (N, N), rows).tolil()
    off = abs(sp.csr_matrix(M)).sum(axis=1).A1 - abs(M.diagonal())
    M.setdiag(rng.choice([-1.0, 1.0], N) * (off + 1.0) * rng.uniform(1.0, 2.0, N))
    return sp.csr_matrix(M)


@functools.lru_cache(maxsize=None)
def ab_case(name):
    build, seed = {"ab_short_rows": (_ab_short_rows, 41), "ab_banded": (_ab_banded, 42)}[name]
    return Case(name, build(np.random.default_rng(seed)), seed)


def ab_compute(mg):
    out = {}
    for name in ("ab_short_rows", "ab_banded"):
        got = device_modes(mg, ab_case(name))
        for key in MODES + ("jacobi2", "jacobi3"):
            out[f"{name}.{key}"] = got[key]
    return out


def ab_child_main(path):
    import agglomerationmultigrid1d_amd as mg
    mg.default_context()
    np.savez(path, **ab_compute(mg))


def run_ab_child(tmp_path, tag, switches):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AGGMG_CSR_")}
    env.update(switches)
    path = str(tmp_path / f"{tag}.npz")
    code = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[2]]; import test_gpu_generic_csr as t; "
            "t.ab_child_main(sys.argv[3])")
    r = subprocess.run([sys.executable, "-c", code, ROOT, os.path.join(ROOT, "tests"), path], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (tag, r.returncode, r.stderr[-3000:])
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def jacobi_sweeps_exact_and_bound(c, ns, alpha=ALPHA):
    """ns point-Jacobi sweeps from c.x: the exact iterate and a bound on a computed one, row by row.

    With T the exact sweep and E_k >= |computed x_k - exact x_k| (E_0 = 0):  computed x_{k+1} is within the one-sweep
    bound of T(computed x_k), evaluated at X = |x_k| + E_k >= |computed x_k| (the bound grows with |x|), and
    |T(v) - T(w)|_i <= |v_i - w_i| + |alpha / d_i| sum_j |a_ij| |v_j - w_j|.  Both added give E_{k+1}."""
    fa = Fraction(alpha)
    n = c.M.shape[0]
    a = [Fraction(float(v)) for v in c.data]
    b = [Fraction(float(v)) for v in c.b]
    d = [Fraction(float(v)) for v in c.diag]
    x = [Fraction(float(v)) for v in c.x]
    E = [Fraction(0)] * n
    for _ in range(ns):
        X = [abs(x[i]) + E[i] for i in range(n)]
        xn, En = [], []
        for i in range(n):
            cols = range(int(c.indptr[i]), int(c.indptr[i + 1]))
            s = sum((a[p] * x[c.indices[p]] for p in cols), Fraction(0))
            SX = sum((abs(a[p]) * X[c.indices[p]] for p in cols), Fraction(0))
            SE = sum((abs(a[p]) * E[c.indices[p]] for p in cols), Fraction(0))
            scale = abs(fa / d[i])
            xn.append(x[i] + fa * (b[i] - s) / d[i])
            En.append(row_bound("jacobi", len(cols), SX, b=b[i], x=X[i], scale=scale) + E[i] + scale * SE)
        x, E = xn, En
    return x, E


def sweeps_outside_bound(c, ns, got):
    ex, E = jacobi_sweeps_exact_and_bound(c, ns)
    if not np.all(np.isfinite(got)):
        return list(range(len(got)))
    return [i for i in range(len(got)) if abs(Fraction(float(got[i])) - ex[i]) > E[i]]


def test_propagated_jacobi_bound_holds_for_the_float64_model():
    """no GPU: 2 and 3 sweeps of the float64 model lie inside the propagated bound on every row of the banded operator,
    and the bound stays far below the iterate (it is not vacuous)"""
    c = ab_case("ab_banded")
    for ns in (2, 3):
        v = c.x
        for _ in range(ns):
            v = v + ALPHA * ((c.b - c.M @ v) / c.diag)
        assert sweeps_outside_bound(c, ns, v) == []
        ex, E = jacobi_sweeps_exact_and_bound(c, ns)
        assert all(E[i] < Fraction(1, 10 ** 9) * (1 + abs(ex[i])) for i in range(len(E)))


@pytest.mark.gpu
def test_ab_switches_give_the_same_results(mg, tmp_path):
    """launch_csr reads AGGMG_CSR_ROWTHREAD once per process, setup_stream_blocks AGGMG_CSR_BAND: each runs in a fresh
    child, one at a time.
    AGGMG_CSR_ROWTHREAD=1: the operator with rows of at most 32 entries and bandwidth > 32 takes csr_rowthread_kernel, the
    banded one csr_rowthread_band_kernel (result vector != x in every mode) -- 'the same bits' as the default stream
    kernel (comments in launch_csr and on csr_rowthread_kernel) in all four modes.
    AGGMG_CSR_BAND=0: the banded operator's 2 and 3 sweeps go one launch each through the stream kernel instead of one
    csr_band_kernel launch; both lie inside the propagated bound, and csr_band_kernel's comment ('S sweeps in one launch
    give bit for bit what S launches give') is held to its word."""
    k = source_constants()
    assert k == BUILT_FOR
    assert not [v for v in os.environ if v.startswith("AGGMG_CSR_")], "the parent has to run the default kernels"
    short, band = ab_case("ab_short_rows"), ab_case("ab_banded")
    assert short.lens.max() == k["rowthread_max"] and bandwidth(short.M) > k["band_max_bw"]
    assert short.M.shape[0] > 2 * k["threads"] and short.M.shape[0] % k["threads"] != 0
    assert band.lens.max() <= k["rowthread_max"] and bandwidth(band.M) == 5 and band.M.shape[0] > k["threads"]
    parent = ab_compute(mg)
    for c in (short, band):
        for mode in MODES:
            assert bad_rows(c, mode, parent[f"{c.name}.{mode}"]) == [], (c.name, mode)
    for ns in (2, 3):
        assert sweeps_outside_bound(band, ns, parent[f"ab_banded.jacobi{ns}"]) == [], ns
    child = run_ab_child(tmp_path, "rowthread", {"AGGMG_CSR_ROWTHREAD": "1"})
    for c in (short, band):
        for mode in MODES:
            key = f"{c.name}.{mode}"
            assert np.array_equal(child[key], parent[key]), key
    child = run_ab_child(tmp_path, "noband", {"AGGMG_CSR_BAND": "0"})
    for ns in (2, 3):
        key = f"ab_banded.jacobi{ns}"
        assert sweeps_outside_bound(band, ns, child[key]) == [], key
        assert np.array_equal(child[key], parent[key]), key
