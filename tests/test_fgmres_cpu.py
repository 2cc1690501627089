"""Flexible GMRES around the V-cycle, the parts that need no GPU: the NumPy model the device loop is compared with
(tests/fgmres_model.py) pins itself -- its history is the minimum of the least-squares problem it claims to solve, and
its iteration counts are the recorded ones -- and the host class of the device loop (csrc/host_gmres.hpp) alone, in a
stand-alone program under AddressSanitizer + UBSan."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from fgmres_model import fgmres_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dg48(oracle):
    return oracle.build_dg_agg_hierarchy(48, p=3, pAgg=1, nAgg=3, first=4)


def test_model_history_is_the_least_squares_minimum(oracle, dg48):
    """V(2,1), restart 8: res never grows, and inside each restart cycle res[j] is min_y ||beta e_1 - Hbar_j y|| of the
    Arnoldi matrix the orthogonalisation produced (numpy.linalg.lstsq), to 1e-10 relative"""
    Ho, _ = dg48
    N = Ho.mStiffness[0].shape[0]
    b = oracle.splitmix_normal(N, 1)
    kept = []
    x, it, res = fgmres_model(oracle, Ho, b, restart=8, maxiter=200, tol=1e-8, nPre=2, nPost=1, kept=kept)
    assert it == len(res) and it > 16                     # (several restart cycles)
    assert all(res[i + 1] <= res[i] for i in range(it - 1))
    assert len(kept) == -(-it // 8)
    for beta, Hbar, first in kept:
        k = Hbar.shape[1]
        assert Hbar.shape == (k + 1, k) and 1 <= k <= 8
        for j in range(k):
            e1 = np.zeros(j + 2)
            e1[0] = beta
            y = np.linalg.lstsq(Hbar[:j + 2, :j + 1], e1, rcond=None)[0]
            ref = np.linalg.norm(e1 - Hbar[:j + 2, :j + 1] @ y)
            assert abs(res[first + j] - ref) <= 1e-10 * ref, (first, j, res[first + j], ref)
    # what the history promises is what the iterate delivers
    nb = np.linalg.norm(b)
    true = np.linalg.norm(b - Ho.mStiffness[0] @ x)
    assert res[-1] < 1e-8 * nb and true <= 1.05e-8 * nb


@pytest.mark.parametrize("restart,count", [(30, 49), (8, 64), (5, 78)])
def test_model_iteration_counts(oracle, dg48, restart, count):
    """dg48 V(2,1) to 1e-8 ||b||: 49 / 64 / 78 iterations at restart 30 / 8 / 5"""
    Ho, _ = dg48
    b = oracle.splitmix_normal(Ho.mStiffness[0].shape[0], 1)
    _, it, _ = fgmres_model(oracle, Ho, b, restart=restart, maxiter=400, tol=1e-8, nPre=2, nPost=1)
    assert it == count


def test_model_modified_gram_schmidt_gives_the_same_count(oracle, dg48):
    Ho, _ = dg48
    b = oracle.splitmix_normal(Ho.mStiffness[0].shape[0], 1)
    _, itc, resc = fgmres_model(oracle, Ho, b, restart=8, maxiter=400, tol=1e-8, nPre=2, nPost=1)
    _, itm, resm = fgmres_model(oracle, Ho, b, restart=8, maxiter=400, tol=1e-8, nPre=2, nPost=1, mgs=True)
    assert itc == itm
    assert np.allclose(resc, resm, rtol=1e-2)


def test_model_edges(oracle, dg48):
    Ho, _ = dg48
    A = Ho.mStiffness[0]
    b = oracle.splitmix_normal(A.shape[0], 1)
    x0 = oracle.splitmix_normal(A.shape[0], 9)
    x, it, res = fgmres_model(oracle, Ho, b, x0=x0, maxiter=0)
    assert it == 0 and res == [] and np.array_equal(x, x0)
    xs, _, _ = fgmres_model(oracle, Ho, b, restart=30, maxiter=200, tol=1e-8, nPre=2, nPost=1)
    x, it, res = fgmres_model(oracle, Ho, b, x0=xs, restart=30, maxiter=200, tol=1e-7, nPre=2, nPost=1)
    assert it == 0 and np.array_equal(x, xs)
    x, it, res = fgmres_model(oracle, Ho, b, restart=1, maxiter=5, tol=1e-8, nPre=2, nPost=1)
    assert it == 5 and all(res[i + 1] <= res[i] for i in range(4))


def test_host_gmres_class_under_asan_ubsan(tmp_path):
    """csrc/host_gmres.hpp alone: tests/host/test_host_gmres.cpp (its own main) compiled with the flags of the SAN line
    of tests/host/Makefile and run as a child process"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mk = open(os.path.join(ROOT, "tests", "host", "Makefile")).read()
    flags = re.search(r"^SAN\s*:=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-fsanitize=address,undefined" in flags
    exe = str(tmp_path / "test_host_gmres")
    src = os.path.join(ROOT, "tests", "host", "test_host_gmres.cpp")
    c = subprocess.run(["g++"] + flags + ["-Werror", "-o", exe, src], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "host_gmres OK" in r.stdout


def test_mirrors_agree_on_fgmres():
    """the Python and the Julia mirror of aggmg_fgmres_dev take the same keywords with the same defaults, and the
    restart bound of the header is the one of _lib and of the host class"""
    from agglomerationmultigrid1d_amd import _lib, api
    import agglomerationmultigrid1d_amd as mg
    assert mg.fgmres is api.fgmres and hasattr(mg.Context, "multi_dot") and hasattr(mg.Context, "multi_axpy_norm")
    py = inspect.signature(api.fgmres).parameters
    assert list(py)[:2] == ["H", "b"]
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    m = re.search(r"^function fgmres\((.*?)\)\n", jl, flags=re.M | re.S)
    assert m, "julia/AggMGHip.jl has no fgmres"
    kws = {}
    for k in re.split(r",(?![^{]*\})", m.group(1).partition(";")[2]):     # (commas outside Union{...})
        name, _, dflt = k.partition("=")
        kws[name.split("::")[0].strip()] = dflt.strip()
    assert sorted(kws) == sorted(k for k in py if k not in ("H", "b"))
    for k, d in kws.items():
        want = py[k].default
        if want is None:
            assert d == "nothing"
        else:
            assert float(eval(d, {"__builtins__": {}})) == float(want), (k, d, want)
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    bound = int(re.search(r"#define AGGMG_FGMRES_MAX_RESTART (\d+)", hdr).group(1))
    host = open(os.path.join(ROOT, "agglomerationmultigrid1d_amd", "csrc", "host_gmres.hpp")).read()
    assert bound == _lib.FGMRES_MAX_RESTART == int(re.search(r"kMaxRestart = (\d+)", host).group(1))
    assert "fgmres" in inspect.getdoc(api.pcg)
