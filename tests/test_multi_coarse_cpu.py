"""CPU-side checks of the column-batched coarsest solve's boundary (aggmg_hier_coarse_solve_multi_dev; EXTENSION: X = A_n \\ B
on K right-hand sides, src/solvers.jl:39,120): the header declares it, the built library exports it, the ctypes table binds
it with the prototype's parameters, and the Julia shim calls it.  No compute calls (no GPU here)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "aggmg_hier_coarse_solve_multi_dev"


def _header():
    txt = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_header_declares_the_entry_point():
    m = re.search(r"\bint\s+" + SYM + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, f"{SYM} is not declared in include/aggmg_hip.h"
    params = [re.sub(r"\s+", " ", p.strip()) for p in m.group(1).split(",")]
    assert params == ["aggmg_ctx* ctx", "aggmg_hier* h", "const double* B", "int64_t ncols", "int64_t ld", "double* X"]


def test_library_exports_it_and_ctypes_binds_it():
    import __graft_entry__ as g
    g.build()
    from agglomerationmultigrid1d_amd import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, SYM), f"{SYM} declared but not exported"
    assert SYM in _lib.SYMBOLS
    ret, args = _lib.SYMBOLS[SYM]
    assert ret is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    assert getattr(_lib.load(), SYM).argtypes == args


def test_python_surfaces_exist():
    import inspect
    from agglomerationmultigrid1d_amd import api
    sig = inspect.signature(api.MeshHierarchy.coarse_solve_multi_dev)
    assert list(sig.parameters) == ["self", "B", "X", "ncols", "ld"]
    assert sig.parameters["ncols"].default is None and sig.parameters["ld"].default is None
    # the exact solutions of multigrid(..., exact=True) on matrices come from one call of the direct solver
    src = inspect.getsource(api._direct_solve_cols)
    assert "solve_dev(dB)" in src and "synchronize" not in src and "for j in" not in src


def test_julia_shim_names_it():
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    code = "\n".join(line.split("#")[0] for line in jl.split("\n"))
    assert re.search(r"ccall\(\(:" + SYM + r",\s*LIB\)", code)
    # the direct solver's `\` on a DeviceMatrix
    assert re.search(r"function\s+Base\.:\\+\(ds::DirectSolver,\s*B::DeviceMatrix\)", code)
    assert re.search(r"function\s+solve\(ds::DirectSolver,\s*A_host,\s*B::DeviceMatrix\)", code)
