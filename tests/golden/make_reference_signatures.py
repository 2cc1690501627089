#!/usr/bin/env python3
"""Generates tests/golden/reference_signatures.json: the signatures of the reference's functions that the Julia shim
extends (tests/test_julia_shim_lint.py, REFERENCE_SIGNATURES), as the lint's own parser reads them from the
reference's text -- for every (file, line) the table names: the function's name, its positional argument count and
its keywords with their defaults.  test_julia_shim_lint checks the table against this file.
Re-run with:  python tests/golden/make_reference_signatures.py <root of the Julia reference tree>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from test_julia_shim_lint import REFERENCE_SIGNATURES, jl_functions  # noqa: E402


def main(ref):
    out = {}
    for name, sigs in REFERENCE_SIGNATURES.items():
        for path, line, _, _ in sigs:
            txt = open(os.path.join(ref, path)).read()
            defs = [d for d in jl_functions(txt) if d[0] == name and d[3] == line]
            if not defs:
                raise SystemExit(f"{path}:{line}: no `function {name}` there")
            _, pos, kws, _ = defs[0]
            out.setdefault(name, []).append({"path": path, "line": line, "npos": len(pos), "keywords": kws})
    with open(os.path.join(HERE, "reference_signatures.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
