"""CPU: bench.py --dump-outputs.  The step's outputs are named by the linear labels (a single tensor "out"), written as float32 .npy, and cut to the
same seeded row subset on every run once they exceed the byte budget; --steps below 1 is refused before anything needs a HIP device."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_small_outputs_are_written_whole(tmp_path):
    g = torch.Generator().manual_seed(0)
    outs = [torch.randn(4, 64, generator=g).half(), torch.randn(2, 3, 32, generator=g).bfloat16()]
    info = bench.write_outputs(bench.output_sample(outs, ["q", "o"]), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["o.npy", "q.npy"]
    q, o = np.load(tmp_path / "q.npy"), np.load(tmp_path / "o.npy")
    assert q.dtype == np.float32 and np.array_equal(q, outs[0].float().numpy())
    assert o.dtype == np.float32 and np.array_equal(o, outs[1].float().reshape(6, 32).numpy())
    assert info["arrays"]["o"] == {"shape": [2, 3, 32], "rows_written": 6}


def test_large_outputs_keep_a_fixed_row_sample_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 10)
    y = torch.randn(1000, 128, generator=torch.Generator().manual_seed(1)).half()
    a, b = bench.output_sample(y, ["unused"]), bench.output_sample(y.clone(), ["unused"])
    assert list(a) == ["out"] and torch.equal(a["out"][0], b["out"][0])
    rows = a["out"][0]
    assert rows.shape == (128, 128) and rows.numel() * 4 <= bench.DUMP_BYTES
    idx = np.sort(np.random.RandomState(0).choice(1000, 128, replace=False))
    assert torch.equal(rows, y.float()[torch.from_numpy(idx)])
    bench.write_outputs(a, str(tmp_path / "d"))
    assert os.path.getsize(tmp_path / "d" / "out.npy") <= bench.DUMP_BYTES + 4096


def test_bench_refuses_fewer_than_one_timed_step():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
