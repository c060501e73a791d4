"""GPU: a plain `bench.py` run does only what its headline figure needs -- set-up, warm-up, the timed steps, one JSON line.  The roofline, CPU-baseline,
fused-QKV and cfg1 / cfg2 / cfg3 / cfg4 / cfg5 blocks are measured only with --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "cpu_baseline", "cfg1", "cfg3", "configs", "step_fused_qkv")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "TOPS" and d["higher_is_better"] is True and d["dtype"] == "int8" and d["value"] > 0 and d["ms_per_step"] > 0
    assert [k for k in FULL_ONLY if k in d] == []
