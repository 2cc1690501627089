"""The coarsest solve's dictionary (AGGMG_OPT_COARSE_DICTIONARY) without a GPU:
 * the stage layout (host_plan.hpp: cr_dict_plan) and the odd record's packing (cr_dict_pack_odd) as a stand-alone
   program under AddressSanitizer + UBSan;
 * the option's number in the header, the ctypes module and the Julia shim, shared with no other option;
 * the new entry points in the header, in the ctypes table and in the front ends, with matching arity."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = ("ERROR: AddressSanitizer", "runtime error:", "ERROR: LeakSanitizer", "SUMMARY: ")
NUMBER = 15


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_dictionary_plan_under_asan_ubsan(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "test_cr_dict_plan")
    src = os.path.join(ROOT, "tests", "host", "test_cr_dict_plan.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert not any(s in r.stderr for s in BAD), r.stderr[-3000:]
    assert "cr_dict_plan OK" in r.stdout


def test_option_number_is_the_same_everywhere():
    from agglomerationmultigrid1d_amd import _lib
    hdr = _read("include", "aggmg_hip.h")
    m = re.search(r"^#define\s+AGGMG_OPT_COARSE_DICTIONARY\s+\((\d+)\)\s*$", hdr, re.M)
    assert m and int(m.group(1)) == NUMBER
    assert _lib.OPT_COARSE_DICTIONARY == NUMBER
    m = re.search(r"^const\s+OPT_COARSE_DICTIONARY\s*=\s*(\d+)\s*$", _read("julia", "AggMGHip.jl"), re.M)
    assert m and int(m.group(1)) == NUMBER
    # no other option has the number, in any of the three (every form of define the header uses)
    nums = re.findall(r"^#define\s+AGGMG_OPT_[A-Z0-9_]+\s+\(?(\d+)\)?", hdr, re.M)
    assert len(nums) == len(set(nums)) and nums.count(str(NUMBER)) == 1
    py = [v for k, v in vars(_lib).items() if k.startswith("OPT_") and isinstance(v, int)]
    assert len(py) == len(set(py))
    jl = re.findall(r"^const\s+OPT_[A-Z0-9_]+\s*=\s*(\d+)\s*$", _read("julia", "AggMGHip.jl"), re.M)
    assert len(jl) == len(set(jl))


def test_entry_points_declared_with_matching_arity():
    from agglomerationmultigrid1d_amd import _lib
    hdr = _read("include", "aggmg_hip.h")
    jl = _read("julia", "AggMGHip.jl")
    for name, nargs, in_julia in (("aggmg_coarse_dictionary_launches", 2, True), ("aggmg_coarse_dictionary_cap", 3, False),
                                  ("aggmg_hier_coarse_dictionary", 9, False)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, f"{name} is not declared in include/aggmg_hip.h"
        assert len(m.group(1).split(",")) == nargs
        assert name in _lib.SYMBOLS, f"{name} is missing from _lib.SYMBOLS"
        assert len(_lib.SYMBOLS[name][1]) == nargs
        if in_julia:
            c = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", jl)
            assert c, f"{name} is not called from julia/AggMGHip.jl"
            assert len([t for t in c.group(1).split(",") if t.strip()]) == nargs


def test_front_ends_and_header_know_the_option():
    from agglomerationmultigrid1d_amd import api
    for name in ("coarse_dictionary_launches", "coarse_dictionary_cap"):
        assert hasattr(api.Context, name)
    assert hasattr(api.MeshHierarchy, "coarse_dictionary") and hasattr(api.MeshHierarchy, "coarse_info")
    hdr = _read("include", "aggmg_hip.h")
    para = " ".join(hdr.split("#define AGGMG_OPT_COARSE_DICTIONARY")[0].rsplit("/*", 1)[1].replace("\n *", "\n").split())
    for word in ("default 56", "AGGMG_COARSE_DICT=0", "bit for bit", "Read when a hierarchy is created",
                 "aggmg_coarse_dictionary_launches", "aggmg_hier_coarse_dictionary"):
        assert word in para, word
    # the cap the header documents is the one host_plan.hpp derives
    assert re.search(r"^constexpr int kCrDictMaxClasses = 56;", _read("agglomerationmultigrid1d_amd", "csrc", "host_plan.hpp"), re.M)
