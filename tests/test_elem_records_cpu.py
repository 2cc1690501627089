"""The packed class records of the element-thread kernels (AGGMG_OPT_ELEMENT_RECORDS_LDS; csrc/host_plan.hpp,
elem_record_pack, reached through aggmg_element_record_pack) without a GPU:
 * every word of a record against the dictionary's arrays it was packed from, in both forms of the transfer's rows
   (second entries of a unit first column / full rows) and with and without the symmetric residual form;
 * pcol = B^{-1} q_{e-1} against the kernels' chain -- row i of the symmetric inverse times q_{e-1}, fma(tri[.], qm[j],
   acc), j ascending, from 0.0 -- with a correctly rounded fma made of exact rational arithmetic;
 * the option's number and the entry points in the header, the ctypes table and the Julia shim."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, T = 4, 10
BSYM, PCOL, QROW, QMIR, DUP, CORR, LF, WORDS = 0, 10, 14, 18, 22, 32, 34, 42   # the header's word offsets


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from agglomerationmultigrid1d_amd import _lib
    return _lib.load()


def _tri(i, j):
    """index of (i, j), i <= j, in the packed upper triangle of a 4 x 4 block (elem_tri<4>)"""
    return i * M - (i * (i - 1)) // 2 + (j - i)


def _fma(a, b, c):
    """a b + c rounded once: exact in rationals, then the correctly rounded conversion"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _pack(lib, nc, bsym, qrow, qmir, dup, corr, lf, lf_unit):
    words = ctypes.c_int(0)
    rec = np.full((max(nc, 1), WORDS), np.nan)
    st = lib.aggmg_element_record_pack(nc, _ptr(bsym), _ptr(qrow), _ptr(qmir), _ptr(dup), _ptr(corr), _ptr(lf), int(lf_unit),
                                       _ptr(rec), ctypes.byref(words))
    assert st == 0 and words.value == WORDS
    return rec[:nc]


def _arrays(nc, seed, lf_unit, sres):
    rng = np.random.default_rng(seed)
    bsym = rng.standard_normal((nc, T)) * np.exp(rng.uniform(-6, 6, (nc, T)))
    qrow = rng.standard_normal((nc, M))
    qmir = rng.standard_normal((nc, M)) * 1e3
    qmir[0] = 0.0                                     # the level's first element has no left neighbour
    dup = rng.standard_normal((nc, T)) if sres else None
    corr = rng.integers(0, 2 ** 32, (nc, M), dtype=np.uint64).astype(np.uint32) if sres else None
    lf = rng.standard_normal((nc, M)) if lf_unit else rng.standard_normal((nc, M, 2))
    return bsym, qrow, qmir, dup, corr, lf


@pytest.mark.parametrize("nc", [1, 7, 32])
@pytest.mark.parametrize("lf_unit,sres", [(True, True), (False, True), (True, False)])
def test_record_words(lib, nc, lf_unit, sres):
    bsym, qrow, qmir, dup, corr, lf = _arrays(nc, 100 * nc + 2 * lf_unit + sres, lf_unit, sres)
    rec = _pack(lib, nc, bsym, qrow, qmir, dup, corr, lf, lf_unit)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert np.array_equal(bits(rec[:, BSYM:BSYM + T]), bits(bsym))
    assert np.array_equal(bits(rec[:, QROW:QROW + M]), bits(qrow))
    assert np.array_equal(bits(rec[:, QMIR:QMIR + M]), bits(qmir))
    if sres:
        assert np.array_equal(bits(rec[:, DUP:DUP + T]), bits(dup))
        assert np.array_equal(np.ascontiguousarray(rec[:, CORR:CORR + 2]).view(np.uint32), corr)
    else:
        assert np.all(bits(rec[:, DUP:LF]) == 0)
    rows = rec[:, LF:LF + 2 * M].reshape(nc, M, 2)
    if lf_unit:
        assert np.all(rows[:, :, 0] == 1.0) and np.array_equal(bits(rows[:, :, 1]), bits(lf))
    else:
        assert np.array_equal(bits(rows), bits(lf))
    # pcol: the kernels' chain, and exactly zero where q_{e-1} is
    for c in range(nc):
        for i in range(M):
            acc = 0.0
            for j in range(M):
                acc = _fma(bsym[c, _tri(min(i, j), max(i, j))], qmir[c, j], acc)
            got = rec[c, PCOL + i]
            assert got == acc and (acc != 0.0 or not np.signbit(got)), (c, i, got, acc)
    assert np.all(bits(rec[0, PCOL:PCOL + M]) == 0)
    assert not np.any(np.isnan(rec))


def test_pcol_is_one_rounding_per_term(lib):
    """operands whose second product needs the fma: rounded on its own it is 1.0 and the sum 0.0"""
    bsym = np.zeros((1, T))
    qmir = np.zeros((1, M))
    e = 2.0 ** -30
    bsym[0, _tri(0, 0)], bsym[0, _tri(0, 1)] = 1.0, 1.0 + e
    qmir[0, 0], qmir[0, 1] = -1.0, 1.0 - e            # -1 + (1 + e)(1 - e) = -e^2, exactly
    rec = _pack(lib, 1, bsym, np.zeros((1, M)), qmir, None, None, np.zeros((1, M)), True)
    assert (1.0 + e) * (1.0 - e) == 1.0
    assert rec[0, PCOL] == -2.0 ** -60
    # row 1 of the symmetric block reads the same word as its column 0: fma(b01, q0, 0) = -(1 + e), then + 0 * q1
    assert rec[0, PCOL + 1] == -(1.0 + e)


def test_bad_arguments(lib):
    words = ctypes.c_int(0)
    assert lib.aggmg_element_record_pack(0, None, None, None, None, None, None, 1, None, ctypes.byref(words)) == 0
    assert words.value == WORDS
    a = np.zeros((1, T))
    assert lib.aggmg_element_record_pack(1, _ptr(a), None, None, None, None, None, 1, None, None) != 0
    assert lib.aggmg_element_record_pack(-1, None, None, None, None, None, None, 1, None, None) != 0


def test_option_and_entry_points_declared():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    for name, nargs in (("aggmg_element_record_lds_launches", 2), ("aggmg_element_record_lds_cap", 3),
                        ("aggmg_element_record_pack", 10)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert len(_lib.SYMBOLS[name][1]) == nargs
    m = re.search(r"^#define\s+AGGMG_OPT_ELEMENT_RECORDS_LDS\s+(\d+)\s*$", hdr, re.M)
    assert m and int(m.group(1)) == _lib.OPT_ELEMENT_RECORDS_LDS == 13
    ids = [int(v) for v in re.findall(r"^#define\s+AGGMG_OPT_[A-Z0-9_]+\s+(\d+)\s*$", hdr, re.M)]
    assert len(ids) == len(set(ids)) and max(ids) == 13
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    assert re.search(r"^const OPT_ELEMENT_RECORDS_LDS = 13\s*$", jl, re.M)
