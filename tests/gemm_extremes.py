"""Int8 GEMM operands whose accumulators leave fp32's exact range, the restated references and arithmetic mutants that go with them, and the tables that
tests/test_gemm_extremes_cpu.py (no GPU) and tests/test_hip_gemm_extremes.py (-m gpu) walk together.  No test functions in here.

Why: with uniform random int8 operands an accumulator is a random walk, max |acc| ~ 2^21 at K = 11008 -- every accumulator and every K-split partial is exact in
fp32, so a kernel that sums partials as floats, converts int32 -> float other than round-to-nearest-even or drops high accumulator bits passes.  The operands built
here put > 80 % of the accumulators beyond +-2^24, both signs, nearly all distinct ("Which outputs see which arithmetic fault").

`python tests/gemm_extremes.py child ENV_NAME CACHE_DIR` is the GPU child of one environment (the library reads its switches once per process);
`python tests/gemm_extremes.py names LIB M,N,K ...` prints asq_gemm_kernel_name of the shapes under this process's environment (query functions only, no GPU)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import detrng  # noqa: E402
from oracle import w8a8 as O  # noqa: E402

F32 = np.float32
SEED = 4242


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# operand builders
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _fractions(stream, n):
    """n agreement fractions from [0.02, 0.2] u [0.8, 0.98]: exactly floor(n / 2) of them in the upper interval, at seeded random positions (so every row / channel
    set, however small, has both signs of 2a - 1)"""
    u = detrng.uniform01(SEED, stream, (n,))
    high = np.zeros(n, bool)
    high[np.argsort(detrng.uniform01(SEED, stream + 1, (n,)), kind="stable")[:n // 2]] = True
    return np.where(high, 0.8 + 0.18 * u, 0.02 + 0.18 * u)


def _signed_rows(stream, frac, p, K):
    """[n, K] of 127 / -128: row i has the sign pattern p on a fraction frac[i] of the positions"""
    agree = detrng.uniform01(SEED, stream, (len(frac), K)) < frac[:, None]
    return np.where(agree == p[None, :], 127, -128).astype(np.int8)


def extreme_operands(M, N, K, tag=0):
    """x int8 [M, K], w int8 [N, K] with acc[m, n] ~ +-15000 K (2 a_m - 1)(2 b_n - 1): a shared sign pattern p[k]; row m agrees with it on a fraction a_m of the
    positions, channel n on b_n; values 127 where the sign is +, -128 where it is -; one activation position in 16 holds a small value in [-32, 31] instead, so the
    low accumulator bits move.  Reproducible (detrng)."""
    s = 16 * tag
    p = detrng.uniform01(SEED, s, (K,)) < 0.5
    x = _signed_rows(s + 1, _fractions(s + 2, M), p, K)
    w = _signed_rows(s + 4, _fractions(s + 5, N), p, K)
    r = detrng.u64(SEED, s + 7, M * K).reshape(M, K)
    small = ((r >> np.uint64(8)) % np.uint64(64)).astype(np.int64) - 32
    x = np.where((r % np.uint64(16)) == 0, small, x).astype(np.int8)
    return x, w


EDGE_K = 130944          # the largest multiple of 128 with 2^14 K < 2^31
EDGE_POS = 2145386496    # (-128)(-128) K
EDGE_NEG = -2128625664   # 127 (-128) K


def edge_operands(M, N, K=EDGE_K, tag=0):
    """extreme_operands plus planted rows / channels of all -128 (index 0) and all 127 (index 1): acc[0, 0] = 2^14 K, acc[1, 0] = acc[0, 1] = -127 * 128 K"""
    x, w = extreme_operands(M, N, K, tag)
    x[0], x[1], w[0], w[1] = -128, 127, -128, 127
    return x, w


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# restated references: every step one separately rounded fp32 numpy operation
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def sat_i8(v):
    with np.errstate(invalid="ignore"):
        return np.clip(np.rint(v.astype(F32)), F32(-128), F32(127)).astype(np.int8)


def ref_i8(acc, alpha, beta=0.0, c=None, accf=None):
    """asq_gemm_i8_i8: sat_i8(rint(alpha f32(acc) + beta f32(c)))"""
    v = (F32(alpha) * (acc.astype(F32) if accf is None else accf)).astype(F32)
    if beta != 0.0:
        v = (v + (F32(beta) * c.astype(F32)).astype(F32)).astype(F32)
    return sat_i8(v)


def ref_q8(acc, s_col, s_row, bias, mid_dt, order, relu, qmode, quant_scale):
    """asq_linear_w8a8_q8 as EpiDequantQ's comment states it: y = DT(dequant(acc) (+ bias)); relu; int8(clamp(rne(y))) or int8(clamp(rne(DT(y / quant_scale))))"""
    y = O.dequant_epilogue(acc, s_col, s_row, bias, mid_dt, order)
    if relu:
        y = np.where(y < 0, F32(0), y).astype(F32)
    return O.act_quant_round(y, mid_dt) if qmode == "per-tensor-round" else O.act_quant_div(y, mid_dt, F32(quant_scale))


def bits(a):
    """bit patterns of a float32 array (so that -0.0 != 0.0 and NaNs compare by payload)"""
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# arithmetic mutants, on the oracle side: what a subtly wrong kernel would compute.  Each returns what replaces f32(acc) (or acc) in the references.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def split_bounds(K, S):
    """the kernels' K-split boundaries: whole 128-wide K-tiles, ceil(nt / S) per split"""
    nt = (K + 127) // 128
    per = (nt + S - 1) // S
    return [(s * per * 128, min((s + 1) * per * 128, K)) for s in range(S) if s * per * 128 < K]


def k_tile_prefix(x, w):
    """int64 [nt + 1, M, N]: exact accumulators over the first t 128-wide K-tiles (a tile's products sum to < 2^21: exact in an fp32 matmul)"""
    K = x.shape[1]
    pre = np.zeros(((K + 127) // 128 + 1,) + (x.shape[0], w.shape[0]), np.int64)
    for t in range(pre.shape[0] - 1):
        pre[t + 1] = pre[t] + (x[:, 128 * t:128 * t + 128].astype(F32) @ w[:, 128 * t:128 * t + 128].astype(F32).T).astype(np.int64)
    return pre


def mutant_split_f32(x, w, S, prefix=None):
    """f32(acc) when the partials of an S-way K split are added as floats"""
    pre = k_tile_prefix(x, w) if prefix is None else prefix
    tot = None
    for (k0, k1) in split_bounds(x.shape[1], S):
        part = (pre[(k1 + 127) // 128] - pre[k0 // 128]).astype(np.int32).astype(F32)
        tot = part if tot is None else (tot + part).astype(F32)
    return tot


def mutant_cvt_rtz(acc):
    """f32(acc) rounded toward zero"""
    f = acc.astype(F32)
    over = np.abs(f.astype(np.float64)) > np.abs(acc.astype(np.float64))
    return np.where(over, np.nextafter(f, F32(0)), f).astype(F32)


def mutant_sext24(acc):
    """acc with its high 8 bits lost: sign-extended from 24 bits"""
    return (((acc.astype(np.int64) & 0xFFFFFF) ^ 0x800000) - 0x800000).astype(np.int32)


def mutant_i8_wrap(acc, alpha):
    """asq_gemm_i8_i8 (beta = 0) when rint(alpha f32(acc)) goes to int32 with wraparound instead of saturation"""
    v = np.rint((F32(alpha) * acc.astype(F32)).astype(F32)).astype(np.float64)
    q = ((v.astype(np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31)
    return np.clip(q, -128, 127).astype(np.int8)


def acc_stats(acc):
    a64 = acc.astype(np.int64)
    inexact = acc.astype(F32).astype(np.float64) != a64.astype(np.float64)
    M, N = acc.shape
    blocks = [bool(inexact[i:i + 16, j:j + 16].any()) for i in range(0, M, 16) for j in range(0, N, 16)]
    return {"inexact": float(inexact.mean()), "pos": float((a64 > 2 ** 24).mean()), "neg": float((a64 < -2 ** 24).mean()), "blocks": all(blocks),
            "log2max": float(np.log2(np.abs(a64).max()))}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the case table
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# name -> (kind, shape).  kind "gemm": (M, N, K); "edge": the int32-edge builder (int32 / fp32 outputs and the int8 entry only); "misaligned": operands one / three
# bytes off 16-byte alignment; "fused": the one-launch forward; "grouped": (counts, N, K)
CASES = {
    "interior": ("gemm", (256, 512, 4096)),       # interior tiles only; persistent-eligible
    "ragged": ("gemm", (300, 520, 4096)),         # ragged M and N; N % 4 == 0, so it splits
    "odd_n": ("gemm", (130, 258, 4096)),          # N % 4 != 0: scalar stores, no split
    "long_k": ("gemm", (128, 256, 16384)),
    "edge": ("edge", (32, 64, EDGE_K)),
    "generic": ("gemm", (37, 52, 4111)),
    "misaligned": ("misaligned", (130, 140, 4096)),
    "row1": ("gemm", (1, 16, 4096)),
    "row17": ("gemm", (17, 1000, 4096)),
    "row64": ("gemm", (64, 4100, 4096)),
    "row100": ("gemm", (100, 200, 4096)),
    "sk70": ("gemm", (70, 260, 8192)),
    "sk128": ("gemm", (128, 16, 16384)),
    "fq4": ("fused", (4, 256, 4096)),
    "fq16": ("fused", (16, 1000, 4096)),
    "g8": ("grouped", ([256] * 8, 256, 4096)),
    "g6": ("grouped", ([300, 0, 17, 256, 1, 511], 320, 4096)),
}
TILED = ("interior", "ragged", "odd_n", "long_k", "edge")
FEW_ROWS = ("row1", "row17", "row64", "row100")
STREAM_K = ("row17", "sk70", "sk128")


# the builder's stream of a case.  row1 has 16 accumulators, too few for fractions of them to hold whatever the stream: its stream is the first of 20 .. 59 at which
# tests/test_gemm_extremes_cpu.py's conditions on the operands all hold (they are conditions on the inputs; no kernel is involved in the choice)
TAGS = {name: i for i, name in enumerate(sorted(CASES))}
TAGS["row1"] = 31


def case_shape(name):
    """(M, N, K) of a case; grouped: (sum of counts, N, K)"""
    kind, s = CASES[name]
    return (sum(s[0]), s[1], s[2]) if kind == "grouped" else s


def case_data(name, cache_dir=None):
    """operands and exact accumulators of a case, computed once per cache_dir: dict(x, w, acc) -- grouped: x [M, K], w [G, N, K], acc [M, N] (each row against its
    group's weight)"""
    path = os.path.join(cache_dir, name + ".npz") if cache_dir else None
    if path and os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] for k in z.files}
    kind, s = CASES[name]
    tag = TAGS[name]
    if kind == "grouped":
        counts, N, K = s
        G, M = len(counts), sum(counts)
        x, w = extreme_operands(M, G * N, K, tag)
        w = w.reshape(G, N, K)
        acc, o = np.empty((M, N), np.int32), 0
        for g, c in enumerate(counts):
            if c:
                acc[o:o + c] = O.igemm(x[o:o + c], w[g])
            o += c
    else:
        x, w = (edge_operands if kind == "edge" else extreme_operands)(*s, tag=tag)
        acc = O.igemm(x, w)
    d = {"x": x, "w": w, "acc": acc}
    if path:
        tmp = path + ".%d.tmp.npz" % os.getpid()
        np.savez(tmp, **d)
        os.replace(tmp, path)
    return d


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the environment table.  env: the switches of the child; cases: what it runs; outs: output sizes in bytes it runs (4: int32 + fp32, 2: fp16 + bf16, 1: the int8
# entries); form: what plan_gemm must answer for (out_bytes, workspace) -- keys of tools/plan_probe.cpp's output, "ksplit": ">1" = any split; "form_<case>" overrides.
# ws: "query" = a workspace of asq_gemm_workspace_bytes where that is > 0 (every child ALSO runs the int32 entry without one); a number = that many scratch bytes.
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _tiled(kern, l16, split=None, ksplit=None, outs=(4, 2, 1), cases=TILED, **more):
    f = {"kern": kern, "l16": l16, "persistent": False}
    with_ws = dict(f, split=split, ksplit=ksplit) if split else dict(f)
    form = {(ob, True): dict(with_ws) for ob in outs}
    form.update({(ob, False): dict(f, ksplit=1, split="none") for ob in outs})
    d = {"cases": cases, "outs": outs, "form": form, "ws": "query", "nosplit": ("odd_n",)}
    d.update(more)
    return d


_SK = {"kern": "skinny", "ws_G": 0}
ENVS = {
    "default": {"env": "", "cases": ("generic", "misaligned", "interior", "ragged") + FEW_ROWS + ("fq4", "fq16", "g8", "g6"), "outs": (4, 2, 1), "ws": "query",
                "form": {(ob, wsf): {} for ob in (4, 2, 1) for wsf in (True, False)},
                "kern": {"generic": "generic", "misaligned": "generic", "interior": "skinny", "ragged": "p8h", "row1": "skinny", "row17": "skinny", "row64": "skinny",
                         "row100": "skinny"}},
    "skinny_nt1": {"env": "ASQ_SK_NT=1", "cases": FEW_ROWS, "outs": (4, 2, 1), "ws": "query",
                   "form": {(ob, wsf): dict(_SK, wide=False) for ob in (4, 2, 1) for wsf in (True, False)}, "mblocks": {"row1": 1, "row17": 1, "row64": 1, "row100": 2}},
    "skinny_nt2": {"env": "ASQ_SK_NT=2", "cases": FEW_ROWS, "outs": (4, 2, 1), "ws": "query",
                   "form": {(ob, wsf): dict(_SK, wide=True) for ob in (4, 2, 1) for wsf in (True, False)}, "mblocks": {"row1": 1, "row17": 1, "row64": 1, "row100": 2}},
    "wstream_nt0": {"env": "ASQ_SK_IMPL=1 ASQ_WS_NT=0", "cases": STREAM_K, "outs": (4, 2, 1), "ws": "query", "stream_k": True,
                    "form": dict([((ob, True), {"kern": "skinny", "ws_G": ">0", "wide": False}) for ob in (4, 2, 1)] + [((ob, False), dict(_SK)) for ob in (4, 2, 1)])},
    "wstream_nt1": {"env": "ASQ_SK_IMPL=1 ASQ_WS_NT=1", "cases": STREAM_K, "outs": (4, 2, 1), "ws": "query", "stream_k": True,
                    "form": dict([((ob, True), {"kern": "skinny", "ws_G": ">0", "wide": True}) for ob in (4, 2, 1)] + [((ob, False), dict(_SK)) for ob in (4, 2, 1)])},
    # gemm_i8_p16 carries 2- and 4-byte outputs; the int8 entries run on p8 in its L16 mode, unsplit without a workspace and in slabs with one (the queries size
    # none for this class, so the child passes 8 MiB of its own)
    "p16": dict(_tiled("p16", False), env="ASQ_GEMM_KERNEL=p16", i8_ws=8 << 20,
                i8_form={False: {"kern": "p8", "l16": True, "ksplit": 1, "split": "none"}, True: {"kern": "p8", "l16": True, "ksplit": ">1", "split": "slabs"}}),
    "p16p": {"env": "ASQ_GEMM_KERNEL=p16 ASQ_P16_PERSIST=2", "cases": ("interior",), "outs": (2,), "ws": "query",
             "form": {(2, True): {"kern": "p16", "persistent": True}, (2, False): {"kern": "p16", "persistent": True}},
             "form_unaligned_out": {"kern": "p16", "persistent": False}},
    # p4x16 carries scalar / per-token scales only: per-channel scales and bias fall back to p16
    "p4x16": dict(_tiled("p4x16", False, outs=(2,), cases=TILED[:4]), env="ASQ_GEMM_KERNEL=p4x16", form_col={"kern": "p16"}),
    "p4": dict(_tiled("p4", False, outs=(2,), cases=TILED[:4]), env="ASQ_GEMM_KERNEL=p4"),
    "p8": dict(_tiled("p8", False, "slabs", ">1"), env="ASQ_GEMM_KERNEL=p8"),
    "p8_split3": dict(_tiled("p8", False, "slabs", 3), env="ASQ_GEMM_KERNEL=p8 ASQ_KSPLIT=3"),
    "p8h": dict(_tiled("p8h", True), env="ASQ_GEMM_KERNEL=p8h"),
    "p8h_mma32": dict(_tiled("p8h", False), env="ASQ_GEMM_KERNEL=p8h ASQ_MMA=32"),
    "p8h_split4": dict(_tiled("p8h", True, "slabs", 4), env="ASQ_GEMM_KERNEL=p8h ASQ_KSPLIT=4"),
    "p8h_split4_mma32": dict(_tiled("p8h", False, "slabs", 4), env="ASQ_GEMM_KERNEL=p8h ASQ_KSPLIT=4 ASQ_MMA=32"),
    "p8q": dict(_tiled("p8q", True), env="ASQ_GEMM_KERNEL=p8q"),
    "p8q_mma32": dict(_tiled("p8q", False), env="ASQ_GEMM_KERNEL=p8q ASQ_MMA=32"),
    # the in-launch reduction (register images, splitk_fix_reduce) carries 2- and 4-byte outputs; int8 outputs go through slabs
    "p8q_split3": dict(_tiled("p8q", True, "in_launch", 3), env="ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=3", i8_form={True: {"kern": "p8q", "l16": True, "ksplit": 3, "split": "slabs"}}),
    "p8q_split3_slabs": dict(_tiled("p8q", True, "slabs", 3), env="ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=3 ASQ_SPLITK_FIX=0"),
    "p8q_split3_mma32": dict(_tiled("p8q", False, "slabs", 3), env="ASQ_GEMM_KERNEL=p8q ASQ_KSPLIT=3 ASQ_MMA=32"),
    "grouped_mma32": {"env": "ASQ_MMA=32", "cases": ("g8", "g6"), "outs": (4, 2), "ws": "query", "form": {}},
}
SWITCHES = ("ASQ_NO_TAIL", "ASQ_SPLITK_FIX", "ASQ_SK_IMPL", "ASQ_GEMM_KERNEL", "ASQ_KSPLIT", "ASQ_MMA", "ASQ_OFFSETS", "ASQ_FUSED_FORWARD", "ASQ_SK_NT", "ASQ_WS_GRID",
            "ASQ_WS_NT", "ASQ_P16_PERSIST", "ASQ_GROUPED_SPLIT", "ASQ_DEBUG_SYNC")


def child_env(env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(kv.split("=", 1) for kv in env.split())
    return e


def expected_form(env_name, case, out_bytes, with_ws, has_col=False, unaligned_out=False):
    """what plan_gemm must answer for one launch of the GPU child (None: a case that does not go through plan_gemm)"""
    e = ENVS[env_name]
    if CASES[case][0] in ("fused", "grouped"):
        return None
    f = dict(e["form"].get((out_bytes, with_ws), {}))
    if out_bytes == 1 and "i8_form" in e and with_ws in e["i8_form"]:
        f = dict(e["i8_form"][with_ws])
    if has_col and "form_col" in e:
        f = dict(e["form_col"])
    if unaligned_out and "form_unaligned_out" in e:
        f = dict(e["form_unaligned_out"])
    if case in e.get("nosplit", ()) and "split" in f:
        f.update(ksplit=1, split="none")
    if "kern" in e and isinstance(e["kern"], dict):
        f["kern"] = e["kern"][case]
    if "mblocks" in e:
        f["mblocks"] = e["mblocks"][case]
    return f


def form_matches(plan, want):
    for k, v in want.items():
        if v == ">1":
            ok = plan[k] > 1
        elif v == ">0":
            ok = plan[k] > 0
        else:
            ok = plan[k] == v
        if not ok:
            return False
    return True


def probe_query(case, out_bytes, has_col, has_bias, scratch, unaligned_out=False):
    M, N, K = case_shape(case)
    aligned = 0 if CASES[case][0] == "misaligned" else 1
    return "%d,%d,%d,%d,%d,%d,%d,%d,%s" % (M, N, K, out_bytes, has_col, has_bias, aligned, 0 if unaligned_out else 1, scratch)


def scratch_arg(env_name, out_bytes, with_ws):
    if not with_ws:
        return "none"
    e = ENVS[env_name]
    return str(e["i8_ws"]) if out_bytes == 1 and "i8_ws" in e else "query"


def run_probe(probe, env, queries):
    r = subprocess.run([probe] + list(queries), env=child_env(env), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(l) for l in r.stdout.splitlines()]


def names_in_child(lib_path, env, shapes):
    """asq_gemm_kernel_name of the real library for the shapes, from a fresh process under `env`"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "names", lib_path] + ["%d,%d,%d" % s for s in shapes], env=child_env(env), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def run_gpu_child(env_name, cache_dir, timeout=240):
    """the GPU child of one environment; returns (returncode, tail of its output).  Nothing retries."""
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "child", env_name, cache_dir]
    r = subprocess.run(cmd, env=child_env(ENVS[env_name]["env"]), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# epilogue operands
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def base_scale(K):
    """a scalar dequant scale that puts |out| at O(1 ... 10^3) for these operands (|acc| ~ 1300 K ... 15000 K)"""
    return F32(1.7e-5 * 4096.0 / K)


def epilogue_operands(M, N, K, tag):
    """s_row [M] in [0.5, 2) with planted rows: two whose scale drives every fp16 output to +-inf while bf16 / fp32 stay finite (one of them negative), one with
    s_row = 0; s_col [N] = base_scale x [0.5, 2); bias [N] ~ 10 N(0, 1)"""
    s_row = (0.5 + 1.5 * detrng.uniform01(SEED + 1, 3 * tag, (M,))).astype(F32)
    rows = {"inf": 0, "neg_inf": M // 2, "zero": M - 1} if M >= 3 else {"inf": 0}
    s_row[rows["inf"]] = F32(3.0e4)
    if M >= 3:
        s_row[rows["neg_inf"]] = F32(-2.5e4)
        s_row[rows["zero"]] = F32(0.0)
    s_col = (base_scale(K) * (0.5 + 1.5 * detrng.uniform01(SEED + 1, 3 * tag + 1, (N,)))).astype(F32)
    bias = (10.0 * detrng.normal(SEED + 1, 3 * tag + 2, (N,))).astype(F32)
    return s_row, s_col, bias, rows


SUBSETS = [(r, c, b) for r in (False, True) for c in (False, True) for b in (False, True)]
ORDERS = ("scale_first", "acc_first")
DTS = {4: ("f32",), 2: ("f16", "bf16")}


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the GPU child
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _child(env_name, cache_dir):
    import torch
    from autosmoothquant_amd import _lib as L, ops
    lib = L.lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    hdr = lib.asq_workspace_header_bytes()
    e = ENVS[env_name]
    TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
    ADT = {"f32": L.ASQ_F32, "f16": L.ASQ_F16, "bf16": L.ASQ_BF16}
    ORD = {"scale_first": L.ASQ_EPI_SCALE_FIRST, "acc_first": L.ASQ_EPI_ACC_FIRST}
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ptr = lambda t: None if t is None else t.data_ptr()

    def make_ws(n):
        if n <= hdr:
            return None, 0
        ws = torch.full((n,), 0x3C, dtype=torch.uint8, device=dev)   # garbage first: the header comes from asq_workspace_init alone
        L.check(lib.asq_workspace_init(ws.data_ptr(), n, st), "init")
        return ws, n

    def tickets_clean(ws):
        return ws is None or int(ws[16:hdr].view(torch.int32).abs().max()) == 0

    def out_buf(M, N, tdt, unaligned=False, fill=None):
        """[M, N] output; unaligned: a contiguous view one element into a larger buffer (data pointer not 16-byte aligned)"""
        buf = torch.empty((M * N + 8,), dtype=tdt, device=dev)
        if fill is not None:
            buf[:] = fill
        elif tdt.is_floating_point:
            buf[:] = float("nan")
        else:
            buf[:] = -7
        o = buf[1:1 + M * N] if unaligned else buf[:M * N]
        assert (o.data_ptr() % 16 != 0) == unaligned
        return o.view(M, N)

    def same(got, ref, what):
        g = got.float().cpu().numpy() if got.dtype.is_floating_point else got.cpu().numpy()
        if g.dtype == F32:
            bad = bits(g) != bits(ref)
        else:
            bad = g != ref
        if bad.any():
            i = np.argwhere(bad)[0]
            raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r" % (what, int(bad.sum()), bad.size, tuple(i), g[tuple(i)], ref[tuple(i)]))

    def gemm_case(name):
        kind, (M, N, K) = CASES[name]
        data = case_data(name, cache_dir)
        x, w, acc = data["x"], data["w"], data["acc"]
        if kind == "misaligned":
            xb, wb = torch.zeros(M * K + 16, dtype=torch.int8, device=dev), torch.zeros(N * K + 16, dtype=torch.int8, device=dev)
            xd, wd = xb[1:1 + M * K].view(M, K), wb[3:3 + N * K].view(N, K)
            xd.copy_(d(x)), wd.copy_(d(w))
            assert xd.data_ptr() % 16 == 1 and wd.data_ptr() % 16 == 3
        else:
            xd, wd = d(x), d(w)
        ws, n = make_ws(lib.asq_gemm_workspace_bytes(M, N, K))
        if e.get("stream_k"):
            assert ws is not None, name
        a = (xd.data_ptr(), wd.data_ptr())
        tag = TAGS[name]
        s_row, s_col, bias, rows = epilogue_operands(M, N, K, tag)
        tr, tc, tb = d(s_row), d(s_col), d(bias)
        accf = acc.astype(F32)
        outs = e["outs"] if kind != "edge" else tuple(o for o in e["outs"] if o != 2)
        # --- int32: twice without a workspace, three times on one workspace
        if 4 in outs:
            for (w_, n_, reps) in ((None, 0, 2), (ws, n, 3)):
                if reps == 3 and ws is None:
                    continue
                for rep in range(reps):
                    out = out_buf(M, N, torch.int32)
                    L.check(lib.asq_gemm_i8_i32(*a, out.data_ptr(), M, N, K, ptr(w_), n_, st), "i32")
                    same(out, acc, "%s i32 ws=%s rep %d" % (name, w_ is not None, rep))
            out = out_buf(M, N, torch.int32, unaligned=True)
            L.check(lib.asq_gemm_i8_i32(*a, out.data_ptr(), M, N, K, ptr(ws), n, st), "i32")
            same(out, acc, name + " i32 unaligned out")
            assert tickets_clean(ws), name + ": tickets not back at zero"

        def linear(dt, s_scalar, r, c, b, order, unaligned=False, w_=ws, n_=n):
            out = out_buf(M, N, TDT[dt], unaligned)
            L.check(lib.asq_linear_w8a8(*a, out.data_ptr(), ADT[dt], M, N, K, float(s_scalar), ptr(tr) if r else None, ptr(tc) if c else None, ptr(tb) if b else None,
                                        ORD[order], ptr(w_), n_, st), "linear_w8a8")
            return out

        # --- the int -> float conversion itself: fp32, unit scale (and 2^-10), no operands; with and without the workspace
        if 4 in outs:
            for sc in (1.0, 2.0 ** -10):
                ref = O.dequant_epilogue(acc, F32(sc), None, None, "f32")
                same(linear("f32", sc, False, False, False, "scale_first"), ref, "%s f32 scale %g" % (name, sc))
                if ws is not None:
                    same(linear("f32", sc, False, False, False, "scale_first", w_=None, n_=0), ref, "%s f32 scale %g, no workspace" % (name, sc))
        # --- the full matrix
        if kind != "edge":
            first = True
            for ob in outs:
                for dt in DTS.get(ob, ()):
                    for (r, c, b) in SUBSETS:
                        for order in ORDERS:
                            ref = O.dequant_epilogue(acc, s_col if c else base_scale(K), s_row if r else None, bias if b else None, dt, order)
                            if first and r:   # the planted rows do what they are there for
                                f16 = O.dequant_epilogue(acc, s_col if c else base_scale(K), s_row, None, "f16", order)
                                assert np.isinf(f16[rows["inf"]]).all() and np.isfinite(O.dequant_epilogue(acc, base_scale(K), s_row, None, "bf16")).all(), name
                                assert len(rows) == 1 or (np.isinf(f16[rows["neg_inf"]]).all() and (f16[rows["zero"]] == 0).all()), name
                                first = False
                            same(linear(dt, base_scale(K), r, c, b, order), ref, "%s %s row=%d col=%d bias=%d %s" % (name, dt, r, c, b, order))
                    # an output whose data pointer is not 16-byte aligned (vec_ok / out_rows16 fallbacks)
                    ref = O.dequant_epilogue(acc, s_col, s_row, bias, dt, "scale_first")
                    same(linear(dt, 1.0, True, True, True, "scale_first", unaligned=True), ref, "%s %s unaligned out" % (name, dt))
                    ref = O.dequant_epilogue(acc, base_scale(K), None, None, dt, "acc_first")
                    same(linear(dt, base_scale(K), False, False, False, "acc_first", unaligned=True), ref, "%s %s unaligned out, scalar scale" % (name, dt))
        # --- the int8 entries
        if 1 in outs:
            c0 = detrng.int8_uniform(SEED + 2, tag, (M, N))
            wss = [(None, 0), (ws, n)] if ws is not None else [(None, 0)]
            if "i8_ws" in e:
                wss.append(make_ws(hdr + e["i8_ws"]))
            alphas = [2.0 ** -18] + ([2.0 ** -18 * 4096.0 / 2 ** int(np.ceil(np.log2(K)))] if K > 4200 else []) + ([4.0] if kind == "edge" else [])
            for (w_, n_) in wss:
                for alpha in alphas:
                    for beta in (0.0, 0.75):
                        for unaligned in ((False, True) if alpha == alphas[0] else (False,)):
                            out = out_buf(M, N, torch.int8, unaligned, fill=0)
                            out.copy_(d(c0))
                            L.check(lib.asq_gemm_i8_i8(*a, out.data_ptr(), M, N, K, alpha, beta, ptr(w_), n_, st), "i8_i8")
                            same(out, ref_i8(acc, alpha, beta, c0, accf), "%s i8 alpha %g beta %g ws=%s unaligned=%d" % (name, alpha, beta, w_ is not None, unaligned))
                if kind != "edge":
                    qsc = F32(base_scale(K) * 0.2)   # |y| at O(0.2 ... 200): about half of the int8 range used, some of it saturated
                    for i, (relu, qmode) in enumerate(((0, "per-tensor-round"), (1, "per-tensor-round"), (0, "per-tensor-div"), (1, "per-tensor-div"))):
                        mid = ("f16", "bf16", "f32", "f16")[i]
                        r, c, b = (i % 2 == 0), (i >= 2), True
                        order = ORDERS[i % 2]
                        qs_col = (s_col * F32(0.2)).astype(F32)
                        q_row = np.where(np.abs(s_row) > 100, F32(1.25), s_row).astype(F32)   # (no +-inf here: inf / NaN through a quantiser is the quantiser tests' subject)
                        out, tq_row, tq_col = out_buf(M, N, torch.int8, fill=0), d(q_row), d(qs_col)
                        L.check(lib.asq_linear_w8a8_q8(*a, out.data_ptr(), ADT[mid], M, N, K, float(qsc), ptr(tq_row) if r else None, ptr(tq_col) if c else None, ptr(tb),
                                                       ORD[order], relu, {"per-tensor-round": L.ASQ_ACT_ROUND, "per-tensor-div": L.ASQ_ACT_DIV}[qmode], 0.731, ptr(w_), n_, st), "q8")
                        ref = ref_q8(acc, qs_col if c else qsc, q_row if r else None, bias, mid, order, relu, qmode, 0.731)
                        same(out, ref, "%s q8 relu=%d %s mid=%s ws=%s" % (name, relu, qmode, mid, w_ is not None))
                assert tickets_clean(w_), name + ": tickets not back at zero (int8 entries)"
        assert tickets_clean(ws), name + ": tickets not back at zero"

    def fused_case(name):
        _, (M, N, K) = CASES[name]
        data = case_data(name, cache_dir)
        x, w, acc = data["x"], data["w"], data["acc"]
        wd = d(w)
        tag = TAGS[name]
        _, s_col, bias, _ = epilogue_operands(M, N, K, tag)
        for dt in ("f32", "f16", "bf16"):
            xf = x.astype(F32)   # integer-valued floats, exact in every dtype: per-tensor-round gives xq = x
            xt = torch.from_numpy(xf).to(TDT[dt]).to(dev)
            for sc in ((1.0, 2.0 ** -10) if dt == "f32" else ()):
                got = ops.linear_w8a8_forward_fused(xt, wd, "per-tensor-round", 1.0, sc)
                same(got, O.dequant_epilogue(acc, F32(sc), None, None, "f32"), "%s fused f32 scale %g" % (name, sc))
            for (c, b) in ((False, False), (True, False), (False, True), (True, True)):
                got = ops.linear_w8a8_forward_fused(xt, wd, "per-tensor-round", 1.0, float(base_scale(K)), d(s_col) if c else None, d(bias) if b else None)
                same(got, O.dequant_epilogue(acc, s_col if c else base_scale(K), None, bias if b else None, dt), "%s fused %s col=%d bias=%d" % (name, dt, c, b))
            # per-token on the same rows: the row scale is 128 / 127 (or 127 / 127) in dt, the quantised rows another set of large accumulators
            xq, qs = O.act_quant_per_token(xf, dt)
            acc_t = O.igemm(xq, w)
            for (c, b) in ((False, False), (True, True)):
                got = ops.linear_w8a8_forward_fused(xt, wd, "per-token", 1.0, float(base_scale(K)), d(s_col) if c else None, d(bias) if b else None)
                same(got, O.dequant_epilogue(acc_t, s_col if c else base_scale(K), qs, bias if b else None, dt), "%s fused per-token %s col=%d bias=%d" % (name, dt, c, b))

    def grouped_case(name):
        _, (counts, N, K) = CASES[name]
        data = case_data(name, cache_dir)
        x, w, acc = data["x"], data["w"], data["acc"]
        G, M = len(counts), sum(counts)
        xd, wd = d(x), d(w)
        tag = TAGS[name]
        s_row, _, _, _ = epilogue_operands(M, N, K, tag)
        sg = (base_scale(K) * (0.5 + 1.5 * detrng.uniform01(SEED + 3, tag, (G,)))).astype(F32)
        gb = (10.0 * detrng.normal(SEED + 3, tag + 100, (G, N))).astype(F32)
        offs = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=dev)
        grp = np.repeat(np.arange(G), counts)
        ws, n = make_ws(lib.asq_grouped_workspace_bytes(M, N, K, G))
        assert ws is not None
        tr, tgb = d(s_row), d(gb)

        def ref_of(sgv, r, b, dt):
            ds = sgv[grp][:, None] if not r else (sgv[grp] * s_row).astype(F32)[:, None]
            out = (ds * acc.astype(F32)).astype(F32)
            if b:
                out = (out + gb[grp]).astype(F32)
            return O.round_to(out, dt)

        def run(sgv, r, b, dt, use_ws):
            out, tsg = out_buf(M, N, TDT[dt]), d(sgv)
            args = (xd.data_ptr(), wd.data_ptr(), out.data_ptr(), ADT[dt], offs.data_ptr(), G, M, N, K, tsg.data_ptr(), ptr(tr) if r else None, ptr(tgb) if b else None)
            if use_ws:
                L.check(lib.asq_linear_w8a8_grouped_ws(*args, ws.data_ptr(), n, st), "grouped_ws")
            else:
                L.check(lib.asq_linear_w8a8_grouped(*args, st), "grouped")
            return out

        for use_ws in (False, True):
            for sc in (1.0, 2.0 ** -10):   # the int -> float conversion itself
                sgv = np.full(G, sc, F32)
                for rep in range(3 if use_ws else 1):
                    same(run(sgv, False, False, "f32", use_ws), ref_of(sgv, False, False, "f32"), "%s grouped f32 scale %g ws=%d rep %d" % (name, sc, use_ws, rep))
            for dt in ("f32", "f16", "bf16"):
                for (r, b) in ((False, False), (True, False), (False, True), (True, True)):
                    same(run(sg, r, b, dt, use_ws), ref_of(sg, r, b, dt), "%s grouped %s row=%d bias=%d ws=%d" % (name, dt, r, b, use_ws))
        assert tickets_clean(ws), name + ": tickets not back at zero"
        got = ops.linear_w8a8_grouped(xd, wd, offs, d(sg), torch.float16, d(s_row), d(gb))   # the module-level wrapper keeps its own workspace
        same(got, ref_of(sg, True, True, "f16"), name + " grouped through ops")

    for name in e["cases"]:
        kind = CASES[name][0]
        {"fused": fused_case, "grouped": grouped_case}.get(kind, gemm_case)(name)
        torch.cuda.synchronize()
        print("case", name, "ok", flush=True)
    print("CHILD OK", env_name)


def _names(lib_path, shapes):
    h = ctypes.CDLL(lib_path)
    h.asq_gemm_kernel_name.restype, h.asq_gemm_kernel_name.argtypes = ctypes.c_char_p, [ctypes.c_int64] * 3
    json.dump([h.asq_gemm_kernel_name(*map(int, s.split(","))).decode() for s in shapes], sys.stdout)


if __name__ == "__main__":
    if sys.argv[1] == "child":
        _child(sys.argv[2], sys.argv[3])
    elif sys.argv[1] == "names":
        _names(sys.argv[2], sys.argv[3:])
