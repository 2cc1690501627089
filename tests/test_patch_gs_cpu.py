"""Multiplicative two-colour element-patch smoother (aggmg_patch_gs_setup, api.ElementPatchGaussSeidel; DESIGN.md
section 20) without a GPU:
 * the NumPy model (tests/patch_gs_model.py): its dense form against its vectorised BlockTridiag form, and the reach of a
   run of sweeps against the halo the planner keeps;
 * the iteration counts of DESIGN.md section 20 as pins of the oracle's cycle and of its pcg_ldiv with the model smoother;
 * the symmetry of the cycle, and that running the post-smoothing forward loses it;
 * the tile planner (host_plan.hpp) as a stand-alone program under AddressSanitizer + UBSan;
 * the three new entry points in the header and in the ctypes table."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import patch_gs_model as gm
import patch_schwarz_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")
ALPHA = 2.0 / 3.0


@pytest.fixture(scope="module")
def h48(oracle):
    return oracle.build_dg_agg_hierarchy(48)


# ---- 1. the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 2, 4])
@pytest.mark.parametrize("ne", [2, 3, 5, 12])
def test_dense_model_is_the_block_tridiagonal_model(oracle, m, ne):
    for coupling in ("dense",) + (("row", "rowcol") if m >= 2 else ()):
        T = pm.random_block_tridiag(m, ne, coupling, 10 * m + ne)
        A = T.tocsc().toarray()
        u, b = oracle.splitmix_normal(m * ne, 3), oracle.splitmix_normal(m * ne, 4)
        for reverse in (False, True):
            for ws in ([1.0], [ALPHA, 0.9, 0.35]):
                want = gm.patch_gs_sweeps(A, m, ne, u, b, ws, reverse)
                got = gm.gs_sweeps(T, u, b, ws, reverse)
                assert np.max(np.abs(got - want)) <= 1e-13 * max(np.max(np.abs(want)), np.max(np.abs(u))), (coupling, reverse, ws)
        # the two directions are different sweeps (ne = 2: one patch, of colour 0 -- the same sweep)
        f, r = gm.gs_sweep(T, u, b, 1.0), gm.gs_sweep(T, u, b, 1.0, reverse=True)
        assert (ne == 2) == bool(np.array_equal(f, r))


def test_model_smoother_is_the_model(oracle, h48):
    H, _ = h48
    for level in (0, 1):
        A = H.mStiffness[level]
        m, ne = pm.level_shape(H, level)
        S = gm.make_model_smoother(oracle, A, m, ne)
        assert isinstance(S, oracle.BlockGaussSeidelRB)
        u, b = oracle.splitmix_normal(m * ne, 11 + level), oracle.splitmix_normal(m * ne, 17 + level)
        # two backward-stable solves of every patch (the oracle's LU, LAPACK's): apart by their condition numbers (the
        # Dirichlet penalty makes the last patch the worst), a factor 16 for the two solves of the sweep's two halves
        Ad = pm.dense(A)
        cond = max(np.linalg.cond(Ad[e * m:(e + 2) * m, e * m:(e + 2) * m]) for e in range(ne - 1))
        for post in (False, True):
            got = oracle.smooth_once(S, A, u, b, ALPHA, post=post)
            want = gm.patch_gs_sweep(A, m, ne, u, b, ALPHA, reverse=post)
            assert np.max(np.abs(got - want)) <= 16 * 2.0 ** -52 * cond * np.max(np.abs(want))


def plan_halo(S):
    return 2 * S + 1   # patch_gs_halo of host_plan.hpp (held to the planner's own by the program below)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_reach_is_the_planners_halo(oracle, S, reverse):
    """perturbing one element changes the elements within the planner's halo and no others; over the two parities the
    halo is reached exactly (one sweep: 3 elements to one side, 2 to the other; two sweeps: 5)"""
    m, ne = 2, 31
    T = pm.random_block_tridiag(m, ne, "dense", 99)
    u, b = oracle.splitmix_normal(m * ne, 5), oracle.splitmix_normal(m * ne, 6)
    base = gm.gs_sweeps(T, u, b, [ALPHA] * S, reverse)
    far = 0
    for at in (14, 15):
        v = u.copy()
        v[at * m:(at + 1) * m] += 1.0
        moved = np.any((gm.gs_sweeps(T, v, b, [ALPHA] * S, reverse) != base).reshape(ne, m), axis=1)
        idx = np.nonzero(moved)[0]
        lo, hi = at - idx.min(), idx.max() - at
        assert max(lo, hi) <= plan_halo(S), (S, reverse, at, lo, hi)
        assert moved[idx.min():idx.max() + 1].all()
        far = max(far, lo, hi)
        if S == 1:   # 3 elements to one side, 2 to the other: which one depends on the parity and the direction
            assert {int(lo), int(hi)} == {2, 3}, (at, reverse, lo, hi)
    assert far == plan_halo(S)


# ---- 2. pins ----------------------------------------------------------------------------------------------------------
def _rows(o, H):
    nl = len(H.mSmoothers)
    return {"defaults": (gm.with_gs_smoothers(o, H, [0]), ALPHA),
            "weight1": (gm.with_gs_smoothers(o, H, [0], {0: 1.0}), ALPHA),
            "all_alpha1": (gm.with_gs_smoothers(o, H, range(nl)), 1.0)}


PINS_48 = {"defaults": ((18, 10), (9, 6), (6, 5)),
           "weight1": ((16, 8), (8, 5), (6, 4)),
           "all_alpha1": ((8, 5), (4, 3), (3, 3))}


@pytest.mark.parametrize("row", sorted(PINS_48))
def test_oracle_counts_n48_p3(oracle, h48, row):
    """cycles of multigrid / iterations of pcg_ldiv to 1e-8 ||b|| for V(1,1), V(2,2), V(3,3), where
    the hybrid patches take 23 / 13 / 9 cycles; the true residual of every pcg result is below the tolerance"""
    H, b = h48
    Hg, alpha = _rows(oracle, H)[row]
    for n, (cyc, its) in zip((1, 2, 3), PINS_48[row]):
        assert gm.cycles_to_tol(oracle, Hg, b, n, n, alpha) == cyc, (row, n)
        it, rel = gm.pcg_its(oracle, Hg, b, n, n, alpha)
        assert it == its and rel < 1e-8, (row, n, it, rel)


def test_hybrid_counts_stay(oracle, h48):
    H, b = h48
    Hp = pm.with_patch_smoothers(oracle, H, [0])
    assert [pm.cycles_to_tol(oracle, Hp, b, n, n) for n in (1, 2, 3)] == [23, 13, 9]


def test_oracle_counts_n256_first8(oracle):
    H, b = oracle.build_dg_agg_hierarchy(256, first=8, nAgg=2)
    assert pm.cycles_to_tol(oracle, pm.with_patch_smoothers(oracle, H, [0]), b, 3, 3) == 27
    Hg = gm.with_gs_smoothers(oracle, H, [0], {0: 1.0})
    assert gm.cycles_to_tol(oracle, Hg, b, 3, 3) == 7
    it, rel = gm.pcg_its(oracle, Hg, b, 3, 3)
    assert it == 5 and rel < 1e-8


# ---- 3. symmetry --------------------------------------------------------------------------------------------------------
def test_cycle_is_symmetric_and_the_direction_matters(oracle, h48):
    H, _ = h48
    for row, (Hg, alpha) in _rows(oracle, H).items():
        for n in (1, 2, 3):
            d = gm.cycle_asymmetry(oracle, Hg, n, alpha)
            assert d <= 1e-10, (row, n, d)
    # forward sweeps in both halves: not symmetric, so the test above sees the direction
    Hg = gm.with_gs_smoothers(oracle, H, [0])
    S = Hg.mSmoothers[0]
    forward = type(S).sweep
    type(S).sweep = lambda self, A, u, b, alpha=1.0, reverse=False: forward(self, A, u, b, alpha, False)
    try:
        for n in (1, 2, 3):
            assert gm.cycle_asymmetry(oracle, Hg, n) > 1e-8, n
    finally:
        type(S).sweep = forward
    # ... and the hybrid cycle is not
    assert gm.cycle_asymmetry(oracle, pm.with_patch_smoothers(oracle, H, [0]), 3) > 1e-8


def test_sweeps_stay_bounded_on_the_random_operators(oracle):
    W = [0.9, 0.35, 0.6, 0.8, 0.45, 0.7, 0.55, 0.65, 0.75, 0.5, 0.85]
    for m, coupling in ((3, "dense"), (4, "row"), (5, "rowcol")):
        T = pm.random_block_tridiag(m, 40, coupling, 8)
        u, b = oracle.splitmix_normal(m * 40, 1), oracle.splitmix_normal(m * 40, 2)
        for ws in ([1.0] * 11, W):
            for reverse in (False, True):
                assert np.max(np.abs(gm.gs_sweeps(T, u, b, ws, reverse))) < 1e3


# ---- 4. planner, ABI --------------------------------------------------------------------------------------------------
def test_patch_gs_planner_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_patch_gs_plan")
    src = os.path.join(ROOT, "tests", "host", "test_patch_gs_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "patch_gs_plan OK" in r.stdout


def test_entry_points_declared_with_matching_arity():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    for name, nargs in (("aggmg_patch_gs_setup", 5), ("aggmg_smoother_patch_kind", 3), ("aggmg_patch_gs_tile_plan", 6)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
        assert len(_lib.SYMBOLS[name][1]) == nargs


def test_front_ends_know_the_smoother():
    import inspect
    from agglomerationmultigrid1d_amd import api, uniform
    assert hasattr(api, "ElementPatchGaussSeidel")
    assert "'patchGS'" in inspect.getsource(api.dg_smoother)
    assert '"patchGS0"' in inspect.getsource(uniform.build_device_hierarchy)
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    assert ":patchGS" in jl and ":aggmg_patch_gs_setup" in jl
