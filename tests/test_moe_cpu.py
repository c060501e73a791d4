"""CPU: the sixth C-ABI header (include/asq_hip_moe.h) and its loader table with the discipline tests/test_attn_extend_cpu.py keeps over the fifth, the argument rules
of its three entries in their stated order (NULL and made-up pointers: nothing is launched), and the yardstick of the GPU tests: tests/moe_ref.py against
MixtralLayer.route on the CPU, its roundings, and the share of weights the 16-bit midpoint exception may claim."""
import os
import re

import numpy as np
import pytest
import torch

import moe_ref as R
from autosmoothquant_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIM, ERR_DTYPE, ERR_ALIGN, ERR_WORKSPACE = 0, -1, -2, -3, -4, -5
MOE_PURE_QUERIES = {"asq_moe_route_workspace_bytes"}      # entries of MOE_SIGNATURES that write no device memory
P, ODD8, ODD4, ODD2 = 1 << 20, (1 << 20) + 8, (1 << 20) + 4, (1 << 20) + 2        # made-up device addresses: 16-byte aligned, 8-, 4- and 2-byte only
HEADERS = ("asq_hip.h", "asq_hip_attn.h", "asq_hip_decode.h", "asq_hip_paged.h", "asq_hip_extend.h")
WEIGHT_SEEDS = (11, 12, 13)                                # tests/test_hip_moe_route.py's seeds for the weight checks
TORCH = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asq_[a-z0-9_]+)\s*\(", src)))


def test_moe_header_and_table_name_the_same_exported_symbols():
    h = L.lib()
    names = _declared("asq_hip_moe.h")
    assert names == ["asq_moe_combine", "asq_moe_dispatch_quantize", "asq_moe_route", "asq_moe_route_workspace_bytes"]
    assert sorted(L.MOE_SIGNATURES) == names
    for n in names:
        assert hasattr(h, n), f"libasq_hip.so lacks {n}"
        fn = getattr(h, n)
        assert (fn.restype, list(fn.argtypes)) == (L.MOE_SIGNATURES[n][0], list(L.MOE_SIGNATURES[n][1]))       # lib() has set it up
    others = set(L.SIGNATURES) | set(L.ATTN_SIGNATURES) | set(L.DECODE_SIGNATURES) | set(L.PAGED_SIGNATURES) | set(L.EXTEND_SIGNATURES)
    assert not set(L.MOE_SIGNATURES) & others
    assert not set(names) & set().union(*(_declared(hd) for hd in HEADERS))
    assert h.asq_version() == L.ASQ_VERSION == 126            # the capability probe is the symbol's presence
    mk = open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", "Makefile")).read()
    assert mk.count("asq_hip_moe.h") == 2 and "asq_moe.hip" in mk      # the header comment and HDRS; the translation unit in SRCS


def test_every_moe_writer_has_a_guard_band_case():
    import test_hip_guardband_moe as T
    covered = {c.entry for c in T.CASES}
    assert MOE_PURE_QUERIES <= set(L.MOE_SIGNATURES) and not (covered & MOE_PURE_QUERIES)
    assert covered <= set(L.MOE_SIGNATURES), sorted(covered - set(L.MOE_SIGNATURES))
    missing = sorted(set(L.MOE_SIGNATURES) - MOE_PURE_QUERIES - covered)
    assert not missing, f"entries of include/asq_hip_moe.h without a guard-band case in tests/test_hip_guardband_moe.py: {missing}"
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert covered == empty, sorted(covered - empty)          # every writer also has its "nothing to do" case
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def test_route_workspace_is_one_histogram_per_block_of_128_tokens():
    ws = L.lib().asq_moe_route_workspace_bytes
    assert ws(0, 8, 2) == ws(-1, 8, 2) == ws(5, 0, 1) == ws(5, 65, 1) == 0
    assert ws(1, 8, 2) == ws(128, 8, 2) == 32 and ws(129, 8, 2) == 64 and ws(1, 1, 1) == 16 and ws(4096, 64, 8) == 32 * 64 * 4
    assert all(ws(T, E, 1) % 16 == 0 and ws(T, E, 1) >= -(-T // 128) * E * 4 for T in (1, 127, 300, 1 << 20) for E in (1, 5, 8, 64))


def _route(T=5, E=8, k=2, ldt=L.ASQ_F16, wdt=L.ASQ_F16, ws_bytes=1 << 10, ptrs=None, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("logits", "sel", "wts", "offs", "tok", "inv", "ws")}
    p.update(named)
    return L.lib().asq_moe_route(p["logits"], ldt, T, E, k, wdt, p["sel"], p["wts"], p["offs"], p["tok"], p["inv"], p["ws"], ws_bytes, None)


def test_route_argument_errors_come_in_the_stated_order():
    h = L.lib()
    for bad in (dict(T=-1), dict(E=0), dict(E=65), dict(E=-3), dict(k=0), dict(k=3, E=2), dict(k=9, E=16), dict(k=9, E=64), dict(T=1 << 31, k=1), dict(T=1 << 30, k=2)):
        assert _route(**bad) == _route(**bad, ptrs=[None], ldt=7) == ERR_DIM, bad                  # 1: dims first, whatever the pointers and codes
        assert b"asq_moe_route" in h.asq_last_error()
    for bad in (dict(ldt=3), dict(wdt=-1), dict(ldt=9, wdt=9)):
        assert _route(**bad) == _route(**bad, ptrs=[None]) == ERR_DTYPE, bad                       # 2: the dtype codes
    assert _route(offs=None) == _route(offs=None, T=0) == _route(ptrs=[None]) == ERR_NULL          # 3: group_offsets is written even for T == 0 ...
    assert _route(offs=ODD2) == _route(offs=ODD2, T=0, ptrs=[None]) == ERR_ALIGN                   # ... and must be an int32 address
    for name in ("logits", "sel", "wts", "tok", "inv"):                                            # 4: NULL before the workspace and the alignment
        assert _route(**{name: None}) == _route(**{name: None}, ws=None, ws_bytes=0) == ERR_NULL, name
    assert _route(ws=None) == _route(ws_bytes=31) == _route(T=129, ws_bytes=63, sel=ODD2) == ERR_WORKSPACE     # 5: the scratch, before the alignment
    for name in ("sel", "wts", "tok", "inv", "ws"):                                                # 6: alignment
        assert _route(**{name: ODD2}) == ERR_ALIGN, name
    assert _route(logits=ODD2 + 1) == _route(logits=ODD2, ldt=L.ASQ_F32) == ERR_ALIGN


def _disp(T=5, k=2, K=64, dt=L.ASQ_F16, mode=L.ASQ_ACT_PER_TOKEN, ptrs=None, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("x", "inv", "xq", "s_row", "row_off")}
    p.update(named)
    return L.lib().asq_moe_dispatch_quantize(p["x"], dt, p["inv"], T, k, K, mode, 0.5, p["xq"], p["s_row"], p["row_off"], None)


def test_dispatch_argument_errors_come_in_the_stated_order():
    h = L.lib()
    for bad in (dict(T=-1), dict(k=0), dict(k=9), dict(K=0), dict(K=-16), dict(T=1 << 31, k=1), dict(T=1 << 30, k=2)):
        assert _disp(**bad) == _disp(**bad, ptrs=[None], dt=5) == ERR_DIM, bad
        assert b"asq_moe_dispatch_quantize" in h.asq_last_error()
    for bad in (dict(dt=3), dict(mode=3), dict(mode=-1)):
        assert _disp(**bad) == _disp(**bad, ptrs=[None]) == ERR_DTYPE, bad
    assert _disp(T=0) == _disp(T=0, ptrs=[None], K=24) == _disp(T=0, ptrs=[ODD2]) == OK                      # nothing to do
    for name in ("x", "inv", "xq"):
        assert _disp(**{name: None}) == _disp(**{name: None}, K=24, ptrs=[ODD2]) == ERR_NULL, name
    assert _disp(s_row=None) == ERR_NULL and _disp(s_row=None, mode=L.ASQ_ACT_ROUND, xq=ODD8) == ERR_ALIGN       # s_row only in per-token mode; row_off may be NULL
    for bad in (dict(K=24), dict(K=8), dict(K=4104), dict(K=16400), dict(K=8208, dt=L.ASQ_F32), dict(K=1 << 20)):
        assert _disp(**bad) == _disp(**bad, ptrs=[ODD2]) == ERR_DIM, bad                                      # K % 16 and the register limit, before the alignment
    for name, addr in (("x", ODD8), ("xq", ODD8), ("row_off", ODD4), ("inv", ODD2), ("s_row", ODD2)):
        assert _disp(**{name: addr}) == ERR_ALIGN, name
    for good in (dict(K=16), dict(K=16384), dict(K=16384, dt=L.ASQ_BF16), dict(K=8192, dt=L.ASQ_F32), dict(k=8), dict(k=1), dict(row_off=None), dict(row_off=ODD8)):
        assert _disp(**good, xq=ODD8) == ERR_ALIGN, good                                                      # accepted by the earlier rules


def _comb(T=5, k=2, H=64, dt=L.ASQ_F16, ptrs=None, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("y", "wts", "inv", "out")}
    p.update(named)
    return L.lib().asq_moe_combine(p["y"], dt, p["wts"], p["inv"], p["out"], T, k, H, None)


def test_combine_argument_errors_come_in_the_stated_order():
    h = L.lib()
    for bad in (dict(T=-1), dict(k=0), dict(k=9), dict(H=0), dict(H=-8), dict(T=1 << 31, k=1), dict(T=1 << 30, k=2), dict(T=(1 << 31) - 1, k=1, H=4096),
                dict(T=(1 << 31) - 1, k=1, H=2048, dt=L.ASQ_F32)):
        assert _comb(**bad) == _comb(**bad, ptrs=[None]) == ERR_DIM, bad
        assert b"asq_moe_combine" in h.asq_last_error()
    assert _comb(dt=3) == _comb(dt=-1, ptrs=[None]) == ERR_DTYPE
    assert _comb(T=0) == _comb(T=0, ptrs=[None], H=12) == OK
    for name in ("y", "wts", "inv", "out"):
        assert _comb(**{name: None}) == _comb(**{name: None}, H=12, ptrs=[ODD2]) == ERR_NULL, name
    for bad in (dict(H=12), dict(H=4), dict(H=6, dt=L.ASQ_F32), dict(H=4100)):
        assert _comb(**bad) == _comb(**bad, ptrs=[ODD2]) == ERR_DIM, bad
    for name, addr in (("y", ODD8), ("out", ODD8), ("wts", ODD2), ("inv", ODD2)):
        assert _comb(**{name: addr}) == ERR_ALIGN, name
    for good in (dict(H=8), dict(H=4, dt=L.ASQ_F32), dict(H=4104), dict(k=8), dict(wts=ODD4, inv=ODD4)):
        assert _comb(**good, out=ODD8) == ERR_ALIGN, good


def test_ops_refuse_cpu_tensors_and_wrong_operands():
    from autosmoothquant_amd import ops
    x, inv, w = torch.zeros(4, 32, dtype=torch.float16), torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4, 2)
    for call in (lambda: ops.moe_route(x, 2, torch.float16), lambda: ops.moe_dispatch_quantize(x, inv, "per-token"), lambda: ops.moe_combine(torch.zeros(8, 32), w, inv)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the reference itself -------------------------------------------------------------------------------------------------------------------
class _Fixed(torch.nn.Module):
    """a router that returns given logits"""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits

    def forward(self, x2):
        return self.logits


def _layer(E, k):
    from autosmoothquant_amd.harness import MixtralLayer
    return MixtralLayer(hidden=32, inter=64, heads=4, kv_heads=2, experts=E, top_k=k)


@pytest.mark.parametrize("E,k", [(8, 2), (5, 1), (64, 8), (8, 8)])
@pytest.mark.parametrize("dt", R.DTS)
def test_reference_agrees_with_mixtral_route_on_gapped_logits(E, k, dt):
    """MixtralLayer.route (softmax over all E in fp32 -> topk -> renormalise -> sort / bincount) with a gate that reproduces given logits: tok, the counts and the
    weights agree with the restated rule -- the weights to the fp32 error of two different but equivalent expressions, then through the same rounding to dt."""
    T = 200
    logits = R.gapped_logits(T, E, 5 + E + k, dt=dt)
    lay = _layer(E, k)
    lay.gate = _Fixed(torch.from_numpy(logits).to(TORCH[dt]))             # (route() only calls it)
    tok, wts, counts = lay.route(torch.zeros(T, 32, dtype=TORCH[dt]))
    ref = R.route(logits, k, dt)
    assert np.array_equal(tok.numpy(), ref["tok"]) and np.array_equal(counts.numpy(), np.diff(ref["group_offsets"]))
    got = wts.float().numpy().astype(np.float64)                          # in sorted-row order
    w64 = ref["w64"].reshape(-1)[np.argsort(ref["inv"].reshape(-1))]
    if dt == "f32":
        assert (np.abs(got - w64) <= 2.0 ** -20 * w64).all()
    else:
        assert (np.abs(got - w64) <= R.ulp_of(w64, dt)).all()
    R.check_safety(ref["sel"], ref["group_offsets"], ref["tok"], ref["inv"], T, E, k)


def test_reference_selection_ties_nan_and_infinities():
    nan, inf = np.nan, np.inf
    l = np.array([[1, 1, 1, 1], [0.0, -0.0, -1, 0.0], [nan, -inf, nan, -3], [inf, nan, inf, 7], [nan, nan, nan, nan], [-inf, -inf, 2, -inf]], np.float32)
    assert R.select(l, 3).tolist() == [[0, 1, 2], [0, 1, 3], [3, 1, 0], [0, 2, 3], [0, 1, 2], [2, 0, 1]]
    r = R.route(l, 3)
    R.check_safety(r["sel"], r["group_offsets"], r["tok"], r["inv"], 6, 4, 3)
    assert r["tok"].tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 2, 4, 5, 0, 3, 4, 5, 1, 2, 3] and r["group_offsets"].tolist() == [0, 6, 11, 15, 18]


def test_reference_roundings():
    x = np.array([1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -7, 1 + 3 * 2.0 ** -8, 0.3, 1e-3], np.float64)
    assert R.round_f64_to(x, "bf16").tolist()[:4] == [1.0, 1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6]              # ties to even
    assert np.array_equal(R.round_f64_to(x, "bf16"), R.bf16_round(x.astype(np.float32)).astype(np.float64))
    assert np.array_equal(R.round_f64_to(x, "f16"), x.astype(np.float16).astype(np.float64))
    assert R.near_midpoint(x, "bf16").tolist() == [False, True, False, True, False, False]
    assert R.near_midpoint(np.array([1 + 2.0 ** -8 + 2.0 ** -21, 1 + 2.0 ** -8 + 2.0 ** -18]), "bf16").tolist() == [True, False]
    assert R.ulp_of(np.array([1.0, 0.75, 0.3]), "f16").tolist() == [2.0 ** -10, 2.0 ** -11, 2.0 ** -12]
    t = torch.tensor([0.1, 0.7, 3.3e-4], dtype=torch.float32)
    assert np.array_equal(R.round_f32_to(t.numpy(), "bf16"), t.bfloat16().float().numpy()) and np.array_equal(R.round_f32_to(t.numpy(), "f16"), t.half().float().numpy())


def test_reference_combine_is_the_fp32_sequence():
    rng = np.random.default_rng(3)
    y = R.round_f32_to(rng.standard_normal((12, 16)).astype(np.float32), "f16")
    inv = rng.permutation(12).astype(np.int32).reshape(4, 3)
    w = R.round_f32_to(rng.uniform(0.1, 0.5, (4, 3)).astype(np.float32), "f16")
    want = torch.zeros(4, 16)
    for j in range(3):
        want = want + torch.from_numpy(y[inv[:, j]]) * torch.from_numpy(w[:, j, None])
    assert np.array_equal(R.combine(y, w, inv, "f16"), want.half().float().numpy())
    assert np.abs(R.combine64(y, w, inv) - R.combine(y, w, inv, "f32")).max() < 1e-6


@pytest.mark.parametrize("seed", WEIGHT_SEEDS)
@pytest.mark.parametrize("dt", ("f16", "bf16"))
def test_midpoint_exception_stays_under_its_cap_for_the_chosen_seeds(seed, dt):
    """the 16-bit weight check of tests/test_hip_moe_route.py excepts weights within 2^-20 (relative) of a rounding midpoint, at most 2 % of them: for its seeds the
    CPU float32 torch composition (softmax -> topk -> renormalise -> .to(dt)) itself differs from round_dt(w64) only inside the exception, by one ulp, and the
    exception claims far less than the cap"""
    from test_hip_moe_route import WEIGHT_CASES, weight_logits
    for (T, E, k) in WEIGHT_CASES:
        logits = weight_logits(T, E, seed, dt)
        ref = R.route(logits, k, dt)
        p = torch.softmax(torch.from_numpy(logits), dim=1, dtype=torch.float)
        w, sel = torch.topk(p, k, dim=-1)
        assert np.array_equal(sel.numpy(), ref["sel"])
        w = (w / w.sum(dim=-1, keepdim=True)).to(TORCH[dt]).float().numpy().astype(np.float64)
        want, near = R.round_f64_to(ref["w64"], dt), R.near_midpoint(ref["w64"], dt)
        differ = w != want
        assert near.mean() <= 0.02 and not (differ & ~near).any(), (T, E, k, near.mean(), int((differ & ~near).sum()))
        assert (np.abs(w - want) <= R.ulp_of(ref["w64"], dt)).all()
