"""CPU: the int8 GEMM dispatcher answers exactly what tests/golden/dispatch_table.json records (tests/golden/make_golden_dispatch.py) -- kernel class,
workspace bytes, offset-image and fused-forward eligibility over 34 row counts x 20 weight shapes, in the default environment and under the switches the
GPU tests and tools force.  The dispatcher is a measured table: a change that moves a row is a deliberate re-measurement (and a re-recorded fixture), never
a side effect of reorganising the launch code."""
import json
import os

import pytest

import dispatch_table as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "dispatch_table.json")) as f:
        g = json.load(f)
    assert g["columns"] == list(D.COLUMNS) and sorted(g["tables"]) == sorted(D.ENVS)
    return g["tables"]


def test_grid_reaches_every_class(golden):
    t = golden[""]
    assert len(t) == len(D.MS) * len(D.NKS) == 680
    assert {r[3] for r in t} == {"skinny", "p8q", "p16", "p8h", "generic", "p16+tail"}
    assert sum(r[4] > 0 for r in t) > 100 and sum(any(r[6]) for r in t) > 100 and sum(any(r[7]) for r in t) >= 40


@pytest.mark.parametrize("env", D.ENVS, ids=[e.replace(" ", ",") or "default" for e in D.ENVS])
def test_library_reproduces_the_recorded_table(golden, env):
    from autosmoothquant_amd import _lib
    got = D.rows_in_child(_lib.LIB_PATH, env)
    want = golden[env]
    assert len(got) == len(want)
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, f"{len(diff)} of {len(want)} rows moved under '{env}'; first (got, recorded): {diff[:3]}"
