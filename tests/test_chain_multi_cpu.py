"""The K-column cycle on CG chain levels (AGGMG_OPT_CHAIN_MULTI) without a GPU:
 * the tile planner (host_plan.hpp: chain_multi_tile_plan) as a stand-alone program under AddressSanitizer + UBSan;
 * the new entry points in the header and in the ctypes table;
 * the option's number in the header, the ctypes module and the Julia shim."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")


def test_chain_multi_planner_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_chain_multi_plan")
    src = os.path.join(ROOT, "tests", "host", "test_chain_multi_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "chain_multi_plan OK" in r.stdout


def test_entry_points_declared_with_matching_arity():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    for name, nargs in (("aggmg_chain_multi_tile_plan", 10), ("aggmg_chain_multi_launches", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
        assert len(_lib.SYMBOLS[name][1]) == nargs
    assert re.search(r"^#define\s+AGGMG_OPT_CHAIN_MULTI\s+\d+\s*$", hdr, re.M), "the option is not in the header"


def test_option_number_is_the_same_everywhere():
    from agglomerationmultigrid1d_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "aggmg_hip.h")).read()
    m = re.search(r"^#define\s+AGGMG_OPT_CHAIN_MULTI\s+(\d+)\s*$", hdr, re.M)
    assert m and int(m.group(1)) == 12
    assert _lib.OPT_CHAIN_MULTI == 12
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    m = re.search(r"^const\s+OPT_CHAIN_MULTI\s*=\s*(\d+)\s*$", jl, re.M)
    assert m and int(m.group(1)) == 12
    # no other option has the number
    nums = re.findall(r"^#define\s+AGGMG_OPT_[A-Z_]+\s+(\d+)\s*$", hdr, re.M)
    assert len(nums) == len(set(nums))


def test_front_ends_know_the_entry_points():
    from agglomerationmultigrid1d_amd import api
    assert hasattr(api.Context, "chain_multi_launches")
    jl = open(os.path.join(ROOT, "julia", "AggMGHip.jl")).read()
    assert ":aggmg_chain_multi_launches" in jl and "function chain_multi_launches(ctx::Context)" in jl
