#!/usr/bin/env python3
"""Records tests/golden/helper_host_contract.json: the call table of tests/test_helper_host_cpu.py (run_table) run on the CPU
against the library that GLSDET_LIB_PATH names -- a build of the commit BEFORE the change under test, never the tree's own:

    GLSDET_LIB_PATH=<parent build>/glsdet_amd/lib/libglsdet_hip.so python tools/make_helper_host_golden.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

if __name__ == "__main__":
    assert os.environ.get("GLSDET_LIB_PATH"), "name the parent commit's library in GLSDET_LIB_PATH"
    from glsdet_amd import _lib
    import test_helper_host_cpu as t
    out = os.path.join(ROOT, "tests", "golden", "helper_host_contract.json")
    with open(out, "w") as f:
        json.dump(t.run_table(_lib.load()), f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", out)
