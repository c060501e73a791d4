#!/usr/bin/env python3
"""Record dispatch_table.json: what the int8 GEMM dispatcher's query functions (kernel class, workspace bytes, offset-image and fused-forward eligibility)
answer over the grid of tests/dispatch_table.py, once per forced environment.  Recorded from the library as built BEFORE a change to the dispatch code;
tests/test_dispatch_table_cpu.py then holds the changed library to it.  A deliberate re-measurement of the dispatcher re-records it.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dispatch.py [path/to/libasq_hip.so]
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dispatch_table as D  # noqa: E402

lib = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "autosmoothquant_amd", "libasq_hip.so")
tables = {env: D.rows_in_child(lib, env) for env in D.ENVS}   # (one child at a time)
with open(os.path.join(HERE, "dispatch_table.json"), "w") as f:
    f.write('{"columns": ' + json.dumps(list(D.COLUMNS)) + ',\n "tables": {\n')
    f.write(",\n".join(json.dumps(env) + ": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in t) + "]" for env, t in tables.items()))
    f.write("}}\n")
for env, t in tables.items():
    print(f"{env or '(default)':40s} {len(t)} rows, classes:", {n: sum(r[3] == n for r in t) for n in sorted({r[3] for r in t})})
