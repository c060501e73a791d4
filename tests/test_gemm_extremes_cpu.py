"""No GPU: the operands of tests/gemm_extremes.py do what tests/test_hip_gemm_extremes.py needs them to do, on the oracle alone.
  (1) every case of the table has accumulators fp32 cannot hold: >= 50 % inexact, >= 40 % beyond each of +-2^24, an inexact one in every 16 x 16 block;
  (2) each arithmetic mutant (K-split partials added as floats, int -> float toward zero, accumulators sign-extended from 24 bits, a wrapping int8 conversion)
      changes the output kind that is meant to see it -- and changes NOTHING on detrng.int8_uniform operands of the same shape, which is what every other oracle
      comparison of the GEMM family feeds the kernels: the gap, written down;
  (3) every (environment, case, output size) of the GPU file reaches the kernel form it is meant to reach: tools/plan_probe.cpp, compiled here, prints plan_gemm's
      answer under each environment; its kernel class is cross-checked against the real library's asq_gemm_kernel_name."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import detrng
import gemm_extremes as GE
from oracle import w8a8 as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
PLAIN = [n for n, (kind, _) in GE.CASES.items() if kind != "grouped"]


@pytest.fixture(scope="module")
def cache(tmp_path_factory):
    return str(tmp_path_factory.mktemp("gemm_extremes"))


def _interior(name, a):
    """the part of an [M, N] array outside the edge builder's planted rows and channels (their accumulators are multiples of 128 below 2^24 against ordinary rows)"""
    return a[2:, 2:] if GE.CASES[name][0] == "edge" else a


@pytest.mark.parametrize("name", list(GE.CASES))
def test_accumulators_leave_fp32(name, cache):
    acc = GE.case_data(name, cache)["acc"]
    st = GE.acc_stats(acc)
    assert st["inexact"] >= 0.5, st
    assert st["pos"] >= 0.4 and st["neg"] >= 0.4, st
    assert st["blocks"], st
    if GE.CASES[name][0] == "edge":
        assert acc[0, 0] == GE.EDGE_POS and acc[1, 0] == GE.EDGE_NEG and acc[0, 1] == GE.EDGE_NEG
        assert int(acc.max()) == GE.EDGE_POS and int(acc.min()) == GE.EDGE_NEG
    else:
        # the planted epilogue rows do what they are there for: fp16 +-inf (bf16 / fp32 finite), and a zero row
        M, N, K = GE.case_shape(name)
        s_row, s_col, bias, rows = GE.epilogue_operands(M, N, K, GE.TAGS[name])
        for sc in (GE.base_scale(K), s_col):
            f16 = O.dequant_epilogue(acc, sc, s_row, None, "f16")
            assert np.isinf(f16[rows["inf"]]).all() and np.isfinite(O.dequant_epilogue(acc, sc, s_row, bias, "bf16")).all()
            if M >= 3:
                assert np.isinf(f16[rows["neg_inf"]]).all() and (f16[rows["zero"]] == 0).all()
                assert (f16[rows["inf"]] > 0).any() and (f16[rows["inf"]] < 0).any()
        mag = np.abs(O.dequant_epilogue(acc, GE.base_scale(K), None, None, "f32"))
        assert 1.0 <= np.median(mag) <= 1e3 and mag.max() <= 2e3     # outputs at O(1 ... 10^3)


def _mutant_effects(name, x, w, acc):
    """fraction of elements each mutant changes, per output kind"""
    M, N, K = GE.case_shape(name)
    f = acc.astype(F32)
    out = {"rtz_f32": GE.bits(GE.mutant_cvt_rtz(acc)) != GE.bits(f), "sext_i32": GE.mutant_sext24(acc) != acc}
    for dt in ("f16", "bf16"):
        out["sext_" + dt] = GE.bits(O.dequant_epilogue(GE.mutant_sext24(acc), GE.base_scale(K), None, None, dt)) != GE.bits(O.dequant_epilogue(acc, GE.base_scale(K), None, None, dt))
    if K % 128 == 0 and w.ndim == 2:
        pre = GE.k_tile_prefix(x, w)
        assert np.array_equal(pre[-1], acc)
        for S in (2, 3, 4, 8):
            out["split%d_f32" % S] = GE.bits(GE.mutant_split_f32(x, w, S, pre)) != GE.bits(f)
    return out


@pytest.mark.parametrize("name", list(GE.CASES))
def test_each_mutant_changes_the_output_that_should_see_it(name, cache):
    d = GE.case_data(name, cache)
    x, w, acc = d["x"], d["w"], d["acc"]
    M, N, K = GE.case_shape(name)
    eff = _mutant_effects(name, x, w, acc)
    # int -> float toward zero: >= 30 % of the unit-scale fp32 output
    assert eff["rtz_f32"].mean() >= 0.3, eff["rtz_f32"].mean()
    # lost high bits: every int32 output, and the fp16 / bf16 outputs (of every row: >= 90 % of the elements)
    assert _interior(name, eff["sext_i32"]).all()
    if GE.CASES[name][0] != "edge":
        for dt in ("f16", "bf16"):
            assert eff["sext_" + dt].mean() >= 0.9 and eff["sext_" + dt].any(axis=1).all(), dt
    # partials added as floats: >= 10 % of the unit-scale fp32 output (measured 13.7 - 35 %), in every row.  A row of 16 channels stays unchanged with probability
    # ~0.8^16 = 3 %, so the every-row condition is asked of outputs at least 64 channels wide (all the shapes the tiled split forms run)
    for S in (2, 3, 4, 8):
        ch = eff.get("split%d_f32" % S)
        if ch is None:
            assert GE.CASES[name][0] == "grouped" or K % 128
            continue
        assert ch.mean() >= 0.1, (S, ch.mean())
        if N >= 64:
            assert _interior(name, ch).any(axis=1).all(), S
    if GE.CASES[name][0] == "edge":
        # alpha acc beyond int32 on > 40 % of the elements; a wrapped value lands on either side of zero, so about half of those differ from the saturated one
        assert (np.abs(4.0 * acc.astype(np.float64)) >= 2.0 ** 31).mean() > 0.4
        assert (GE.mutant_i8_wrap(acc, 4.0) != GE.ref_i8(acc, 4.0)).mean() > 0.2
        assert np.array_equal(GE.mutant_i8_wrap(acc, 2.0 ** -23), GE.ref_i8(acc, 2.0 ** -23))   # (the mutant is the reference where nothing overflows)


@pytest.mark.parametrize("name", PLAIN)
def test_no_mutant_changes_anything_on_uniform_operands(name):
    """detrng.int8_uniform operands of the same shape: an accumulator is a random walk that stays below 2^23, so every mutant computes the reference's bits --
    a kernel with any of these faults passes every comparison made on such operands"""
    M, N, K = GE.case_shape(name)
    x, w = detrng.int8_uniform(101, M * 7 + K, (M, K)), detrng.int8_uniform(102, N * 5 + K, (N, K))
    acc = O.igemm(x, w)
    assert np.abs(acc.astype(np.int64)).max() < 2 ** 23
    eff = _mutant_effects(name, x, w, acc)
    assert eff and not any(v.any() for v in eff.values()), {k: float(v.mean()) for k, v in eff.items()}
    assert np.array_equal(GE.mutant_i8_wrap(acc, 4.0), GE.ref_i8(acc, 4.0))


# ---- (3) the kernel forms
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")) if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path_factory.mktemp("plan_probe") / "plan_probe")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "autosmoothquant_amd", "csrc"), os.path.join(ROOT, "tools", "plan_probe.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


def _queries(env_name):
    """every launch kind of the GPU child that goes through plan_gemm: (query, expected form)"""
    e = GE.ENVS[env_name]
    qs = []
    for case in e["cases"]:
        if GE.CASES[case][0] in ("fused", "grouped"):
            continue
        for ob in e["outs"]:
            if GE.CASES[case][0] == "edge" and ob == 2:
                continue
            for with_ws in (False, True):
                sc = GE.scratch_arg(env_name, ob, with_ws)
                qs.append((GE.probe_query(case, ob, 0, 0, sc), GE.expected_form(env_name, case, ob, with_ws)))
                if "form_col" in e:
                    qs.append((GE.probe_query(case, ob, 1, 1, sc), GE.expected_form(env_name, case, ob, with_ws, has_col=True)))
                if "form_unaligned_out" in e:
                    qs.append((GE.probe_query(case, ob, 0, 0, sc, unaligned_out=True), GE.expected_form(env_name, case, ob, with_ws, unaligned_out=True)))
    return qs


@pytest.mark.parametrize("env_name", list(GE.ENVS))
def test_every_environment_reaches_its_kernel_form(env_name, probe):
    from autosmoothquant_amd import _lib
    e = GE.ENVS[env_name]
    qs = _queries(env_name)
    if not qs:
        assert all(GE.CASES[c][0] in ("fused", "grouped") for c in e["cases"])
        return
    plans = GE.run_probe(probe, e["env"], [q for q, _ in qs])
    assert len(plans) == len(qs)
    for (q, want), plan in zip(qs, plans):
        assert plan["nparts"] == 1, (q, plan)
        assert GE.form_matches(plan, want), (env_name, q, want, plan)
    # the probe answers as the library does: kernel class of the int32 caps against asq_gemm_kernel_name, in a child under the same environment
    shapes = sorted({GE.case_shape(c) for c in e["cases"] if GE.CASES[c][0] == "gemm" or GE.CASES[c][0] == "edge"})
    if shapes:
        names = GE.names_in_child(_lib.LIB_PATH, e["env"], shapes)
        got = GE.run_probe(probe, e["env"], ["%d,%d,%d,4,0,0,1,1,query" % s for s in shapes])
        assert names == [p["cls_any"] for p in got] == [p["cls"] for p in got], (names, got)


def test_tables_cover_the_forms():
    """the environments reach, between them, every kernel form the issue lists"""
    envs = " | ".join(e["env"] for e in GE.ENVS.values())
    for kern in ("p16", "p4x16", "p4", "p8", "p8h", "p8q"):
        assert "ASQ_GEMM_KERNEL=" + kern in envs
    for sw in ("ASQ_P16_PERSIST=2", "ASQ_SK_NT=1", "ASQ_SK_NT=2", "ASQ_SK_IMPL=1 ASQ_WS_NT=0", "ASQ_SK_IMPL=1 ASQ_WS_NT=1", "ASQ_GEMM_KERNEL=p8 ASQ_KSPLIT=3",
               "ASQ_GEMM_KERNEL=p8h ASQ_KSPLIT=4", "ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=3 ASQ_SPLITK_FIX=0", "ASQ_MMA=32"):
        assert sw in envs, sw
    want = {(256, 512, 4096), (300, 520, 4096), (130, 258, 4096), (128, 256, 16384), (32, 64, 130944), (37, 52, 4111), (130, 140, 4096), (1, 16, 4096),
            (17, 1000, 4096), (64, 4100, 4096), (100, 200, 4096), (70, 260, 8192), (128, 16, 16384), (4, 256, 4096), (16, 1000, 4096)}
    assert want <= {GE.case_shape(n) for n in GE.CASES}
    assert all(K >= 4096 for (_, _, K) in map(GE.case_shape, GE.CASES))     # (K = 2048 gives only 34 % fp32-inexact accumulators)
    used = {c for e in GE.ENVS.values() for c in e["cases"]}
    assert used == set(GE.CASES)
