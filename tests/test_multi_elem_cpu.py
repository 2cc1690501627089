"""The K-column element-thread launches (AGGMG_OPT_MULTI_ELEMENT_THREADS) without a GPU:
 * the library exports the counter, the per-level query and the planner; the option's number in the header, the ctypes
   module and the Julia shim;
 * aggmg_multi_element_tile_plan is the fused launches' planner on a tile of 256 elements: owned =
   floor((256 - 2 halo) / rho) rho, 0 where the halo eats the tile;
 * the same planner from host_plan.hpp as a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")
NUMBER = 16
SYMBOLS = (("aggmg_multi_element_thread_launches", 2), ("aggmg_hier_level_multi_element_threads", 7),
           ("aggmg_multi_element_tile_plan", 4))
TILE = 256
# (halo, rho): the descent of V(3,3) and of V(2,.) into agglomerates of 4, V(8,8)'s descent, an ascent of one sweep beside a
# ratio of 2, a halo that leaves nothing; then the edges of the formula
PLAN_CASES = [(4, 4), (3, 4), (9, 4), (1, 2), (128, 4), (0, 1), (8, 1), (127, 1), (127, 2), (126, 4), (126, 8), (5, 3), (200, 1)]


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_library_exports_the_symbols():
    from agglomerationmultigrid1d_amd import _lib
    lib = _lib.load()
    for name, nargs in SYMBOLS:
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    assert _lib.OPT_MULTI_ELEMENT_THREADS == NUMBER


def test_option_number_is_the_same_everywhere():
    from agglomerationmultigrid1d_amd import _lib
    hdr = _read("include", "aggmg_hip.h")
    m = re.search(r"^#define\s+AGGMG_OPT_MULTI_ELEMENT_THREADS\s+\((\d+)\)\s*$", hdr, re.M)
    assert m and int(m.group(1)) == NUMBER
    m = re.search(r"^const\s+OPT_MULTI_ELEMENT_THREADS\s*=\s*(\d+)\s*$", _read("julia", "AggMGHip.jl"), re.M)
    assert m and int(m.group(1)) == NUMBER
    nums = re.findall(r"^#define\s+AGGMG_OPT_[A-Z0-9_]+\s+\(?(\d+)\)?", hdr, re.M)
    assert len(nums) == len(set(nums)) and nums.count(str(NUMBER)) == 1
    py = [v for k, v in vars(_lib).items() if k.startswith("OPT_") and isinstance(v, int)]
    assert len(py) == len(set(py))


def test_entry_points_declared_with_matching_arity():
    hdr = _read("include", "aggmg_hip.h")
    src = _read("agglomerationmultigrid1d_amd", "csrc", "aggmg_hip.hip")
    jl = _read("julia", "AggMGHip.jl")
    for name, nargs in SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert re.search(r'^extern "C" int %s\(' % name, src, re.M), name
    c = re.search(r"ccall\(\(:aggmg_multi_element_thread_launches, LIB\), Cint,\s*\(([^)]*)\)", jl)
    assert c and len([t for t in c.group(1).split(",") if t.strip()]) == 2
    assert "function multi_element_thread_launches(ctx::Context)" in jl


def test_front_ends_and_header_know_the_option():
    from agglomerationmultigrid1d_amd import api
    assert hasattr(api.Context, "multi_element_thread_launches")
    assert hasattr(api.MeshHierarchy, "multi_element_thread_levels")
    hdr = _read("include", "aggmg_hip.h")
    para = " ".join(hdr.split("#define AGGMG_OPT_MULTI_ELEMENT_THREADS")[0].rsplit("/*", 1)[1].replace("\n *", "\n").split())
    for word in ("default 0", "AGGMG_MULTI_ELEM_THREADS=1", "bit for bit", "Read at every call", "aggmg_multi_element_thread_launches",
                 "aggmg_hier_level_multi_element_threads", "aggmg_multi_element_tile_plan"):
        assert word in para, word


@pytest.mark.parametrize("halo,rho", PLAN_CASES)
def test_tile_plan_is_the_fused_planner_on_256_elements(halo, rho):
    from agglomerationmultigrid1d_amd import _lib
    lib = _lib.load()
    te, owned = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.aggmg_multi_element_tile_plan(halo, rho, ctypes.byref(te), ctypes.byref(owned)) == 0
    want = max(0, (TILE - 2 * halo) // rho) * rho
    assert te.value == TILE and owned.value == want and owned.value % rho == 0, (halo, rho, te.value, owned.value, want)
    assert (owned.value == 0) == (TILE - 2 * halo < rho)


def test_tile_plan_figures_of_the_cycles():
    """what the halves of V(3,3), V(2,.) and V(8,8) into agglomerates of 4 and an ascent of one sweep own, from the formula"""
    from agglomerationmultigrid1d_amd import _lib
    lib = _lib.load()
    got = {}
    for halo, rho in PLAN_CASES[:5]:
        te, owned = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.aggmg_multi_element_tile_plan(halo, rho, ctypes.byref(te), ctypes.byref(owned)) == 0
        got[halo, rho] = owned.value
    assert got == {(h, r): max(0, (TILE - 2 * h) // r) * r for h, r in PLAN_CASES[:5]}
    assert got == {(4, 4): 248, (3, 4): 248, (9, 4): 236, (1, 2): 254, (128, 4): 0}


def test_tile_plan_refuses_bad_arguments():
    from agglomerationmultigrid1d_amd import _lib
    lib = _lib.load()
    te, owned = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.aggmg_multi_element_tile_plan(-1, 4, ctypes.byref(te), ctypes.byref(owned)) == _lib.ERR_ARGUMENT
    assert lib.aggmg_multi_element_tile_plan(4, 0, ctypes.byref(te), ctypes.byref(owned)) == _lib.ERR_ARGUMENT
    assert lib.aggmg_multi_element_tile_plan(4, 4, None, ctypes.byref(owned)) == _lib.ERR_ARGUMENT


def test_planner_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_multi_elem_plan")
    src = os.path.join(ROOT, "tests", "host", "test_multi_elem_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "multi_elem_plan OK" in r.stdout
