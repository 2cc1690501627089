"""fgmres_multi without a GPU: the Python and Julia mirrors of aggmg_fgmres_multi_dev agree, the header and _lib list the
new entry points, and the slot bookkeeping of the lockstep loop (csrc/host_gmres_cols.hpp) is tested alone, in a
stand-alone program under AddressSanitizer + UBSan."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("aggmg_fgmres_multi_dev", "aggmg_multi_dot_cols_dev", "aggmg_multi_axpy_norm_cols_dev")


def _julia_keywords(jl, name):
    """keyword -> default text of `function name(...; ...)` (the parsing of test_mirrors_agree_on_fgmres)"""
    m = re.search(r"^function %s\((.*?)\)\n" % re.escape(name), jl, flags=re.M | re.S)
    assert m, f"julia/AggMGHip.jl has no {name}"
    kws = {}
    for k in re.split(r",(?![^{]*\})", m.group(1).partition(";")[2]):     # (commas outside Union{...})
        kname, _, dflt = k.partition("=")
        kws[kname.split("::")[0].strip()] = dflt.strip()
    return kws, m.group(0)


def test_mirrors_agree_on_fgmres_multi():
    from agglomerationmultigrid1d_amd import api
    import agglomerationmultigrid1d_amd as mg
    assert mg.fgmres_multi is api.fgmres_multi
    assert hasattr(mg.Context, "multi_dot_cols") and hasattr(mg.Context, "multi_axpy_norm_cols")
    assert hasattr(mg.MeshHierarchy, "fgmres_multi_dev")
    py = inspect.signature(api.fgmres_multi).parameters
    assert list(py)[:2] == ["H", "B"]
    want = dict(X0=None, restart=30, maxiter=200, tol=1e-10, nPre=3, nPost=3, alpha=2.0 / 3.0)
    assert {k: p.default for k, p in py.items() if k not in ("H", "B")} == want
    dev = inspect.signature(mg.MeshHierarchy.fgmres_multi_dev).parameters
    assert list(dev)[:3] == ["self", "B", "X"]
    assert {k: p.default for k, p in dev.items() if k not in ("self", "B", "X")} == \
        dict(ncols=None, ld=None, **{k: v for k, v in want.items() if k != "X0"})
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    kws, _ = _julia_keywords(jl, "fgmres_multi")
    assert sorted(kws) == sorted(want)
    for k, d in kws.items():
        if want[k] is None:
            assert d == "nothing"
        else:
            assert float(eval(d, {"__builtins__": {}})) == float(want[k]), (k, d, want[k])
    body = jl[jl.index("function fgmres_multi("):]
    body = body[:body.index("\nend\n")]
    assert "GC.@preserve" in body and ":aggmg_fgmres_multi_dev" in body


def test_fgmres_keeps_its_signature_and_names_fgmres_multi():
    """a name of its own: fgmres takes what it took, and says where K right-hand sides go"""
    from agglomerationmultigrid1d_amd import api
    py = inspect.signature(api.fgmres).parameters
    assert list(py) == ["H", "b", "x0", "restart", "maxiter", "tol", "nPre", "nPost", "alpha"]
    assert "fgmres_multi" in inspect.getdoc(api.fgmres)
    assert "One right-hand side only" not in inspect.getdoc(api.fgmres)
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    kws, _ = _julia_keywords(jl, "fgmres")
    assert sorted(kws) == sorted(k for k in py if k not in ("H", "b"))


def test_header_and_lib_list_the_entry_points():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    src = open(os.path.join(ROOT, "agglomerationmultigrid1d_amd", "csrc", "aggmg_hip.hip")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(aggmg_ctx\* ctx" % name, hdr, flags=re.M), name
        assert re.search(r'^extern "C" int %s\(' % name, src, flags=re.M), name
        assert name in _lib.SYMBOLS, name
    # the argument count of the ctypes entry is the one of the declaration
    for name in NEW_SYMBOLS:
        decl = re.search(r"^int %s\((.*?)\);" % name, hdr, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SYMBOLS[name][1]), name


def test_slot_bookkeeping_under_asan_ubsan(tmp_path):
    """csrc/host_gmres_cols.hpp alone: tests/host/test_host_gmres_cols.cpp (its own main) compiled with the flags of the
    SAN line of tests/host/Makefile and run as a child process"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    mk = open(os.path.join(ROOT, "tests", "host", "Makefile")).read()
    flags = re.search(r"^SAN\s*:=\s*(.+)$", mk, flags=re.M).group(1).split()
    assert "-fsanitize=address,undefined" in flags
    exe = str(tmp_path / "test_host_gmres_cols")
    src = os.path.join(ROOT, "tests", "host", "test_host_gmres_cols.cpp")
    c = subprocess.run(["g++"] + flags + ["-Werror", "-o", exe, src], capture_output=True, text=True, timeout=600)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert "host_gmres_cols OK" in r.stdout
