"""K-column hybrid / additive patch sweeps and the option that puts them into the K-column cycle
(AGGMG_OPT_PATCH_SCHWARZ_MULTI) without a GPU:
 * the tile planner (host_plan.hpp: patch_schwarz_multi_tile_plan) as a stand-alone program under AddressSanitizer + UBSan;
 * the new entry points in the header, in the ctypes table and in the Julia shim, with matching arity;
 * the option's number in the header, the ctypes module and the Julia shim."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")
NUMBER = 14


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_patch_schwarz_multi_planner_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_patch_schwarz_multi_plan")
    src = os.path.join(ROOT, "tests", "host", "test_patch_schwarz_multi_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "patch_schwarz_multi_plan OK" in r.stdout


def test_option_number_is_the_same_everywhere():
    from agglomerationmultigrid1d_amd import _lib
    hdr = _read("include", "aggmg_hip.h")
    m = re.search(r"^#define\s+AGGMG_OPT_PATCH_SCHWARZ_MULTI\s+(\d+)\b", hdr, re.M)
    assert m and int(m.group(1)) == NUMBER
    assert _lib.OPT_PATCH_SCHWARZ_MULTI == NUMBER
    m = re.search(r"^const\s+OPT_PATCH_SCHWARZ_MULTI\s*=\s*(\d+)\s*$", _read("julia", "AggMGHip.jl"), re.M)
    assert m and int(m.group(1)) == NUMBER
    # no other option has the number, in any of the three
    # (every define of an option, with or without a comment behind the number)
    nums = re.findall(r"^#define\s+AGGMG_OPT_[A-Z0-9_]+\s+(\d+)\b", hdr, re.M)
    assert len(nums) == len(set(nums)) and str(NUMBER) in nums and len(nums) == NUMBER
    py = [v for k, v in vars(_lib).items() if k.startswith("OPT_") and isinstance(v, int)]
    assert len(py) == len(set(py))
    jl = re.findall(r"^const\s+OPT_[A-Z0-9_]+\s*=\s*(\d+)\s*$", _read("julia", "AggMGHip.jl"), re.M)
    assert len(jl) == len(set(jl))


def test_entry_points_declared_with_matching_arity():
    from agglomerationmultigrid1d_amd import _lib
    hdr = _read("include", "aggmg_hip.h")
    jl = _read("julia", "AggMGHip.jl")
    for name, nargs, in_julia in (("aggmg_patch_schwarz_multi_tile_plan", 7, False), ("aggmg_patch_schwarz_multi_launches", 2, True),
                                  ("aggmg_smooth_multi_dev", 11, True)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
        assert len(_lib.SYMBOLS[name][1]) == nargs
        if in_julia:   # the shim's ccall: return type, a tuple of nargs argument types, nargs arguments
            c = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", jl)
            assert c, f"{name} is not called from julia/AggMGHip.jl"
            assert len([t for t in c.group(1).split(",") if t.strip()]) == nargs
    # the planner's signature is the multiplicative one's
    assert _lib.SYMBOLS["aggmg_patch_schwarz_multi_tile_plan"] == _lib.SYMBOLS["aggmg_patch_gs_multi_tile_plan"]


def test_front_ends_know_the_entry_points():
    import inspect
    from agglomerationmultigrid1d_amd import api
    assert hasattr(api.Context, "patch_schwarz_multi_launches")
    got = list(inspect.signature(api.ElementPatchSchwarz.sweeps_multi_dev).parameters)
    assert got == ["self", "U0", "B", "U", "weights", "ncols", "ld"], got
    jl = _read("julia", "AggMGHip.jl")
    assert "function patch_schwarz_multi_launches(ctx::Context)" in jl
    assert "function sweeps_multi(S::DeviceSmoother" in jl and "OPT_PATCH_SCHWARZ_MULTI" in jl.split("function sweeps_multi(")[0][-400:]


def test_header_documents_the_option_and_the_ignored_direction():
    hdr = _read("include", "aggmg_hip.h")
    para = hdr.split("#define AGGMG_OPT_PATCH_SCHWARZ_MULTI")[0].rsplit("/*", 2)[1]
    for word in ("default 0", "AGGMG_PATCH_SCHWARZ_MULTI=1", "bit for bit", "Read at", "aggmg_patch_schwarz_multi_launches"):
        assert word in " ".join(para.replace("\n *", "\n").split()), word
    doc = " ".join(hdr.split("int aggmg_smooth_multi_dev(")[0].rsplit("/*", 1)[1].replace("\n *", "\n").split())
    assert "AGGMG_OPT_PATCH_SCHWARZ_MULTI" in doc and "`reverse` is accepted and ignored" in doc
