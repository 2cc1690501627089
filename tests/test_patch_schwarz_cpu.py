"""Element-patch Schwarz smoother (aggmg_patch_schwarz_setup, api.ElementPatchSchwarz) without a GPU:
 * the NumPy model of the sweep (tests/patch_schwarz_model.py) against the oracle's HybridSchwarzSmoother on the element-patch
   lists, and the lists themselves;
 * the iteration counts of DESIGN.md section 19 as pins of the oracle's cycle with that smoother;
 * the tile planner of the fused sweep kernel (host_plan.hpp) as a stand-alone program under AddressSanitizer + UBSan;
 * the two new entry points in the header and in the ctypes table."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import patch_schwarz_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")


@pytest.fixture(scope="module")
def h48(oracle):
    return oracle.build_dg_agg_hierarchy(48)


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("hybrid", [True, False])
def test_model_is_the_oracles_schwarz_smoother_on_the_lists(oracle, h48, level, hybrid):
    H, _ = h48
    A = H.mStiffness[level]
    m, ne = pm.level_shape(H, level)
    assert (m, ne) == ((4, 48) if level == 0 else (2, 12))
    S = pm.oracle_patch_smoother(oracle, A, m, ne, hybrid=hybrid)
    u = oracle.splitmix_normal(m * ne, 11 + level)
    b = oracle.splitmix_normal(m * ne, 17 + level)
    want = u + S.apply(b - oracle.csc_matvec(A, u), 2.0 / 3.0)
    got = pm.patch_sweep(A, m, ne, u, b, 2.0 / 3.0, hybrid)
    assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want))


def test_lists_and_counts():
    for m in (1, 2, 4):
        for ne in (3, 5, 12):
            L = pm.patch_lists(m, ne)
            assert L.shape == (2 * m, ne - 1)
            for e in range(ne - 1):
                assert np.array_equal(L[:, e], np.arange(e * m + 1, (e + 2) * m + 1))
            c = pm.patch_counts(m, ne).reshape(ne, m)
            assert np.all(c[0] == 1) and np.all(c[-1] == 1) and np.all(c[1:-1] == 2)
        assert np.array_equal(pm.patch_lists(m, 1), np.arange(1, m + 1)[:, None])       # ne = 1: one patch {0}
        assert np.all(pm.patch_counts(m, 1) == 1)
        assert np.array_equal(pm.patch_lists(m, 2), np.arange(1, 2 * m + 1)[:, None])   # ne = 2: one patch {0, 1}
        assert np.all(pm.patch_counts(m, 2) == 1)
    # the package builds the same lists
    from agglomerationmultigrid1d_amd.api import element_patch_lists
    for m, ne, w in ((3, 7, 2), (2, 5, 3), (4, 2, 4), (1, 1, 2)):
        assert np.array_equal(element_patch_lists(m, ne, w), pm.patch_lists(m, ne, w))


def test_oracle_counts_n48_p3(oracle, h48):
    """9 / 23 / 16 cycles of V(3,3) / V(1,1) / V(2,1) with the patch smoother on level 0 where
    block-Jacobi takes 72; patches on every smoothed level give the same V(3,3) count"""
    H, b = h48
    assert pm.cycles_to_tol(oracle, H, b) == 72
    Hp = pm.with_patch_smoothers(oracle, H, [0])
    assert pm.cycles_to_tol(oracle, Hp, b, 3, 3) == 9
    assert pm.cycles_to_tol(oracle, Hp, b, 1, 1) == 23
    assert pm.cycles_to_tol(oracle, Hp, b, 2, 1) == 16
    assert pm.cycles_to_tol(oracle, pm.with_patch_smoothers(oracle, H, range(len(H.mSmoothers))), b) == 9


@pytest.mark.parametrize("p,count", [(1, 7), (2, 8)])
def test_oracle_counts_lower_order(oracle, p, count):
    H, b = oracle.build_dg_agg_hierarchy(48, p=p)
    assert pm.cycles_to_tol(oracle, pm.with_patch_smoothers(oracle, H, [0]), b) == count


def test_patch_planner_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_patch_plan")
    src = os.path.join(ROOT, "tests", "host", "test_patch_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "patch_plan OK" in r.stdout


def test_entry_points_declared_with_matching_arity():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    for name, nargs in (("aggmg_patch_schwarz_setup", 7), ("aggmg_smoother_patch_info", 5)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
        assert len(_lib.SYMBOLS[name][1]) == nargs
