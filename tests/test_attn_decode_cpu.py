"""CPU: the third C-ABI header (include/asq_hip_decode.h) and its loader table with the discipline tests/test_rope_q8_cpu.py keeps over the second, the argument
rules of asq_attn_decode_i8 and asq_rope_quantize_qkv_at in their stated order (NULL and made-up pointers: nothing is launched), the refusals of the ops and the
modules, RaggedInt8KVCache's bookkeeping, and the yardstick of the GPU test: tests/attn_decode_ref.py's chunk() pinned to the constants of csrc/asq_attn_decode.hip
and to DESIGN.md 4.12's figures, its caps for every case and sign, its intervals collapsing to exact values on the constructed cases (uniform, one-hot per r and per D,
the key-position walk for 4 / 8 / 16 waves, the two weights under both signs), and the teeth of those cases: the float32 model chunked_probs() passes every
constructed and chunked case as it is and is rejected on a named case with each of its five defects."""
import os
import re

import numpy as np
import pytest
import torch

import attn_decode_ref as R
from autosmoothquant_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIM, ERR_DTYPE, ERR_ALIGN = 0, -1, -2, -3, -4
F32, F16, BF16 = L.ASQ_F32, L.ASQ_F16, L.ASQ_BF16
DECODE_PURE_QUERIES = set()      # entries of DECODE_SIGNATURES that write no device memory: none
P, ODD, ODD4 = 1 << 20, (1 << 20) + 8, (1 << 20) + 2        # made-up device addresses: 16-byte aligned, 8-byte only, 2-byte only


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asq_[a-z0-9_]+)\s*\(", src)))


def test_decode_header_and_table_name_the_same_exported_symbols():
    h = L.lib()
    names = _declared("asq_hip_decode.h")
    assert names == ["asq_attn_decode_i8", "asq_rope_quantize_qkv_at"]
    assert sorted(L.DECODE_SIGNATURES) == names
    for n in names:
        assert hasattr(h, n), f"libasq_hip.so lacks {n}"
        fn = getattr(h, n)
        assert (fn.restype, list(fn.argtypes)) == (L.DECODE_SIGNATURES[n][0], list(L.DECODE_SIGNATURES[n][1]))     # lib() has set it up
    assert not set(L.DECODE_SIGNATURES) & (set(L.SIGNATURES) | set(L.ATTN_SIGNATURES))
    assert not set(names) & (set(_declared("asq_hip.h")) | set(_declared("asq_hip_attn.h")))
    assert h.asq_version() == L.ASQ_VERSION == 126            # the capability probe is the symbol's presence
    mk = open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", "Makefile")).read()
    assert "asq_hip_decode.h" in mk and "asq_attn_decode.hip" in mk


def test_every_decode_writer_has_a_guard_band_case():
    import test_hip_guardband_decode as T
    covered = {c.entry for c in T.CASES}
    assert DECODE_PURE_QUERIES <= set(L.DECODE_SIGNATURES) and not (covered & DECODE_PURE_QUERIES)
    assert covered <= set(L.DECODE_SIGNATURES), sorted(covered - set(L.DECODE_SIGNATURES))
    missing = sorted(set(L.DECODE_SIGNATURES) - DECODE_PURE_QUERIES - covered)
    assert not missing, f"entries of include/asq_hip_decode.h without a guard-band case in tests/test_hip_guardband_decode.py: {missing}"
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert covered == empty, sorted(covered - empty)          # every writer also has its "nothing to do" case
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def _dec(B=2, Hq=4, Hkv=2, D=16, pitch=0, ml=8, ptrs=None, kv_len=P, **named):
    """asq_attn_decode_i8 with sane small arguments except those given; ptrs: one value for q / k / v / out, named: one of them alone"""
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "out")}
    p.update(named)
    return L.lib().asq_attn_decode_i8(p["q"], p["k"], p["v"], kv_len, p["out"], B, Hq, Hkv, D, pitch, ml, 0.01, 0.02, None)


def test_decode_argument_errors_come_in_the_stated_order():
    h = L.lib()
    bad_dims = [dict(B=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(D=257), dict(D=272), dict(ml=-1), dict(ml=1 << 17), dict(B=1 << 31), dict(Hq=1 << 31),
                dict(B=(1 << 31) - 1, Hkv=(1 << 31) - 1, Hq=(1 << 31) - 1)]
    for bad in bad_dims:                                        # 1: dims first, whatever the pointers
        assert _dec(**bad) == _dec(**bad, ptrs=[None]) == ERR_DIM, bad
        assert b"asq_attn_decode_i8" in h.asq_last_error()
    for e in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(Hq=0, Hkv=0)):                                            # 2: nothing to do
        assert _dec(**e, ptrs=[None]) == _dec(**e, ptrs=[ODD], D=24, pitch=5, kv_len=ODD4) == OK, e
    for name in ("q", "k", "v", "out"):                         # 3: NULL before the shape rules and the alignment; kv_len may be NULL
        assert _dec(**{name: None}) == _dec(**{name: None}, D=24, pitch=5, ptrs=[ODD]) == ERR_NULL, name
    assert _dec(kv_len=None, ptrs=[ODD]) == ERR_ALIGN
    bad_shape = [dict(D=24), dict(D=8), dict(Hq=5), dict(Hq=3, Hkv=2), dict(Hq=34, Hkv=2), dict(Hq=17, Hkv=1),
                 dict(pitch=16), dict(pitch=8 * 2 * 16 - 16), dict(pitch=8 * 2 * 16 + 8), dict(pitch=-16)]          # below max_len * Hkv * D = 256; no multiple of 16
    for bad in bad_shape:                                       # 4: the shape rules before the alignment
        assert _dec(**bad) == _dec(**bad, ptrs=[ODD], kv_len=ODD4) == ERR_DIM, bad
    for name in ("q", "k", "v", "out"):                         # 5: alignment, 16 B for the tensors and 4 B for kv_len
        assert _dec(**{name: ODD}) == ERR_ALIGN, name
    assert _dec(kv_len=ODD4) == ERR_ALIGN and b"kv_len" in h.asq_last_error()
    for good in (dict(Hq=32, Hkv=2), dict(Hq=16, Hkv=1), dict(D=256), dict(pitch=256), dict(pitch=272), dict(ml=0), dict(ml=(1 << 17) - 1), dict(kv_len=None), dict(kv_len=P + 4)):
        assert _dec(**good, out=ODD) == ERR_ALIGN, good            # accepted by rules 1 - 4: seen as the next rule's code


def _at(dt=F16, B=1, S=2, Hq=2, Hkv=1, D=16, T=8, qp=0, kp=0, vp=0, kvb=0, ml=8, ptrs=None, pos=P, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "cos", "sin", "q8", "kc", "vc")}
    p.update(named)
    return L.lib().asq_rope_quantize_qkv_at(p["q"], p["k"], p["v"], qp, kp, vp, dt, p["cos"], p["sin"], T, pos, p["q8"], p["kc"], p["vc"], kvb, ml, 0.37, 0.11, 0.73,
                                            B, S, Hq, Hkv, D, None)


def test_append_argument_errors_come_in_the_stated_order():
    h = L.lib()
    names = ("q", "k", "v", "cos", "sin", "q8", "kc", "vc")
    bad_dims = [dict(B=-1), dict(S=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(T=-1), dict(ml=-1), dict(ml=1 << 31), dict(S=1 << 31), dict(Hq=1 << 31),
                dict(D=1 << 20), dict(B=(1 << 31) - 1, S=(1 << 31) - 1, Hq=(1 << 31) - 2), dict(B=1 << 20, S=1 << 20, Hq=64, D=128)]
    for bad in bad_dims:                                        # 1: dims first -- whatever the dtype and the pointers
        assert _at(**bad) == _at(**bad, dt=7, ptrs=[None], pos=None) == ERR_DIM, bad
        assert b"asq_rope_quantize_qkv_at" in h.asq_last_error()
    assert _at(dt=7, ptrs=[None]) == _at(dt=-1, B=0) == _at(dt=3, D=24, ptrs=[ODD]) == ERR_DTYPE        # 2: then the dtype, also for an empty problem
    for e in (dict(B=0), dict(S=0), dict(Hq=0), dict(Hkv=0)):                                            # 3: nothing to do
        for dt in (F32, F16, BF16):
            assert _at(**e, dt=dt, ptrs=[None], pos=None) == _at(**e, dt=dt, ptrs=[ODD], D=24, qp=3, kvb=5, pos=ODD4) == OK, e
    for name in names:                                          # 4: NULL, pos included, before the shape rules and the alignment
        assert _at(**{name: None}) == _at(**{name: None}, D=24, qp=3, kvb=5, ptrs=[ODD]) == ERR_NULL, name
    assert _at(pos=None) == _at(pos=None, D=24, ptrs=[ODD]) == ERR_NULL
    bad_shape = [(dict(D=24), F16), (dict(D=8), BF16), (dict(D=12), F32), (dict(qp=16), F16), (dict(kp=8), F16), (dict(vp=8), F16), (dict(qp=36), F16), (dict(qp=34), F32),
                 (dict(kvb=16), F16), (dict(kvb=8 * 16 - 16), F16), (dict(kvb=8 * 16 + 8), F16), (dict(kvb=32, ml=3), BF16)]      # the pitch rule is max_len's, not S's
    for bad, dt in bad_shape:                                   # 5: the shape rules before the alignment
        assert _at(**bad, dt=dt) == _at(**bad, dt=dt, ptrs=[ODD], pos=ODD4) == ERR_DIM, (bad, dt)
    for name in names:                                          # 6: every pointer's alignment, 4 B for pos
        assert _at(**{name: ODD}) == ERR_ALIGN, name
    assert _at(pos=ODD4) == ERR_ALIGN and b"pos" in h.asq_last_error()
    for good, dt in [(dict(D=8), F32), (dict(kvb=128), F16), (dict(kvb=144), F16), (dict(kvb=32, ml=2), F16), (dict(T=0), F16), (dict(T=1), F16), (dict(ml=0), F16),
                     (dict(pos=P + 4), BF16)]:                  # positions beyond the tables are the device's business: no host rule
        assert _at(**good, dt=dt, ptrs=[ODD]) == ERR_ALIGN, (good, dt)


def _i8(*s):
    return torch.zeros(s, dtype=torch.int8)


def test_ops_and_modules_refuse_cpu_tensors_bad_strides_and_wide_groups():
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, RaggedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, smax = 2, 4, 2, 16, 8
    q, kc, vc, n = _i8(B, Hq, D), _i8(B, smax, Hkv, D), _i8(B, smax, Hkv, D), torch.zeros(B, dtype=torch.int32)
    for args, kw in (((q, kc, vc, n), {}), ((q.view(B, 1, Hq, D), kc[:, :5], vc[:, :5], None), {}), ((q, kc, vc, n), dict(max_len=3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.attn_decode_i8(*args, 0.01, 0.02, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Int8Attention(0.01, 0.02).decode(q.view(B, 1, Hq, D), kc, vc, n)
    bad = [
        dict(q=q.float()), dict(q=q[0]), dict(q=_i8(B, 2, Hq, D)), dict(q=_i8(B, Hq, 2 * D)[..., :D]), dict(q=_i8(B + 1, Hq, D)),
        dict(q=_i8(B, 34, D)),                                  # r = 17
        dict(q=_i8(B, 5, D)),                                   # Hq no multiple of Hkv
        dict(q=_i8(B, Hq, 24), k_cache=_i8(B, smax, Hkv, 24), v_cache=_i8(B, smax, Hkv, 24)),      # D no multiple of 16
        dict(k_cache=kc.transpose(1, 2)), dict(k_cache=kc[:, ::2], v_cache=vc[:, ::2]), dict(k_cache=_i8(B, smax, Hkv, 2 * D)[..., :D]),
        dict(k_cache=kc[:, :5]),                                # the two caches disagree
        dict(v_cache=_i8(B, 2 * smax, Hkv, D)[:, :smax]),       # two batch pitches
        dict(v_cache=vc.to(torch.int16)), dict(k_cache=_i8(smax, B, Hkv, D).transpose(0, 1), v_cache=_i8(smax, B, Hkv, D).transpose(0, 1)),
        dict(kv_len=n.long()), dict(kv_len=torch.zeros(B + 1, dtype=torch.int32)), dict(kv_len=[1, 2]),
        dict(max_len=smax + 1), dict(max_len=-1),
    ]
    for kw in bad:
        a = dict(q=q, k_cache=kc, v_cache=vc, kv_len=n, max_len=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_decode_i8(a["q"], a["k_cache"], a["v_cache"], a["kv_len"], 0.01, 0.02, max_len=a["max_len"])
    with pytest.raises(ValueError):
        Int8Attention(0.01, 0.02).decode(q, kc, vc, n)          # the module takes [B, 1, Hq, d]
    # the append: rope_quantize_qkv's stride rules, an int32 [B] pos, two caches of one shape and pitch
    z = lambda *s: torch.zeros(s, dtype=torch.float16)  # noqa: E731
    S, T = 3, 8
    fq, fk, fv, cos, sin = z(B, S, Hq, D), z(B, S, Hkv, D), z(B, S, Hkv, D), z(T, D // 2), z(T, D // 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rope_quantize_qkv_at(fq, fk, fv, cos, sin, 0.37, 0.11, 0.73, n, kc, vc)
    for kw in (dict(q=fq.transpose(1, 2)), dict(k=fk.float()), dict(v=fv[:, :2]), dict(cos=cos[:, :4]), dict(pos=n.long()), dict(pos=torch.zeros(3, dtype=torch.int32)),
               dict(pos=0), dict(k_cache=kc[:, :5]), dict(k_cache=kc[:, ::2], v_cache=vc[:, ::2]), dict(v_cache=_i8(B, smax, Hkv + 1, D)), dict(k_cache=kc[:1], v_cache=vc[:1])):
        a = dict(q=fq, k=fk, v=fv, cos=cos, sin=sin, pos=n, k_cache=kc, v_cache=vc)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.rope_quantize_qkv_at(a["q"], a["k"], a["v"], a["cos"], a["sin"], 0.37, 0.11, 0.73, a["pos"], a["k_cache"], a["v_cache"])
    mod, cache = RopeQuantQKV(0.37, 0.11, 0.73), RaggedInt8KVCache(B, smax, Hkv, D)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(fq, fk, fv, cos, sin, cache=cache)
    assert cache.lengths == [0, 0] and cache.kv_len.tolist() == [0, 0]          # a refused call does not advance the cache
    cache.advance([6, 0])
    with pytest.raises(ValueError):
        mod(fq, fk, fv, cos, sin, cache=cache)                  # 3 more tokens do not fit the first sequence: refused before anything is launched
    with pytest.raises(ValueError):
        mod(fq[:, :1], fk[:, :1], fv[:, :1], cos, sin, cache=cache, advance=[3, 1])
    assert cache.lengths == [6, 0]
    assert sorted(Int8Attention(0.01, 0.02).state_dict()) == ["pv_bmm.a", "qk_bmm.a"]          # decode() adds no state


def test_ragged_cache_bookkeeping():
    from autosmoothquant_amd.layers.nn.attention import RaggedInt8KVCache
    c = RaggedInt8KVCache(3, 8, 2, 16, device="cpu")
    assert c.k.shape == c.v.shape == (3, 8, 2, 16) and c.k.dtype == c.v.dtype == torch.int8 and c.k.data_ptr() != c.v.data_ptr() and c.max_len == 8
    assert c.kv_len.dtype == torch.int32 and c.kv_len.tolist() == c.lengths == [0, 0, 0] and c.bound() == 0
    ptr = c.kv_len.data_ptr()
    c.advance(2)
    assert c.kv_len.tolist() == c.lengths == [2, 2, 2]
    c.advance([5, 0, 1])
    assert c.kv_len.tolist() == c.lengths == [7, 2, 3] and c.bound() == 7
    for bad in (2, [0, 0, 6], [1, 1], [-1, 0, 0], -1):
        with pytest.raises(ValueError):
            c.advance(bad)
    assert c.kv_len.tolist() == c.lengths == [7, 2, 3]          # a refused advance moves nothing
    c.advance([1, 6, 5])
    assert c.lengths == [8, 8, 8] and c.bound() == 8
    c.reset(1)
    assert c.kv_len.tolist() == c.lengths == [8, 0, 8]
    c.reset(-1)
    assert c.kv_len.tolist() == c.lengths == [8, 0, 0]
    c.k.fill_(7)
    c.reset()
    assert c.kv_len.tolist() == c.lengths == [0, 0, 0] and bool((c.k == 7).all())       # reset() forgets, it does not clear
    assert c.kv_len.data_ptr() == ptr                           # the device tensor a captured step reads stays where it is


def _constant(src, name):
    expr = re.search(rf"constexpr int {name} = ([^;]+);", src).group(1)
    assert re.fullmatch(r"[0-9A-Z_ ()+*]+", expr), expr
    return expr


def test_chunk_restates_dec_chunk_and_the_documented_figures():
    src = open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", "asq_attn_decode.hip")).read()
    pad = int(_constant(src, "DEC_PAD"))
    strip = eval(_constant(src, "DEC_STRIP_BYTES"), {"DEC_PAD": pad})
    assert (pad, strip) == (R.DEC_PAD, R.DEC_STRIP_BYTES), "the strip budget of asq_attn_decode.hip moved: tests/attn_decode_ref.py restates it, and every edge case is derived from it"
    body = src[src.index("inline int dec_chunk(int r, int64_t max_len)"):]
    body = body[:body.index("}")]
    assert "fit = (DEC_STRIP_BYTES / (4 * r) - DEC_PAD) / 64 * 64" in body and "need = max_len < 64 ? 64 : (max_len + 63) / 64 * 64" in body and "need < fit ? need : fit" in body
    top = R.MAX_LEN_LIMIT
    assert "max_len < (1ll << 17)" in src and top == (1 << 17) - 1
    assert [R.chunk(r, top) for r in (16, 12, 8, 7, 4, 3, 1)] == [1024, 1344, 2048, 2304, 4096, 5440, 16384]       # 1024 at r = 16, 4096 at r = 4
    assert "(1024 keys at r = 16, 4096 at r = 4, never" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for r in range(1, 17):
        fit = R.chunk(r, top)
        assert fit % 64 == 0 and 4 * r * (fit + pad) <= strip < 4 * r * (fit + 64 + pad)
        assert [R.chunk(r, n) for n in (0, 1, 64, 65, fit - 1, fit, fit + 1)] == [64, 64, 64, 128, fit, fit, fit]
    # what the case tables promise about themselves
    forms = {((R.CASES[ci][2] + 63) // 64, R.chunked(ci)) for ci in range(len(R.CASES))}
    assert forms == {(nd, ch) for nd in (1, 2, 3, 4) for ch in (False, True)}
    assert {R.CASES[ci][1] for ci in range(len(R.CASES))} >= {1, 2, 3, 4, 5, 6, 7, 8, 12, 16}
    assert sorted({ci for ci, _ in R.NEG_PARAMS}) == [ci for ci in range(R.NEW_CASES, len(R.CASES)) if max(R.CASES[ci][3]) > R.chunk(R.CASES[ci][1], max(R.CASES[ci][3]) + 3)]
    assert len({ci for ci, _ in R.NEG_PARAMS}) == 6
    for ci in R.POISONED[2:]:
        assert R.chunked(ci)


SIGNED = [(p, 1) for p in R.PARAMS] + [(p, -1) for p in R.NEG_PARAMS]


@pytest.mark.parametrize("p,sign", SIGNED, ids=[R.param_id(p) + ("-neg" if sign < 0 else "") for p, sign in SIGNED])
def test_the_yardstick_keeps_its_caps_on_every_gpu_case(p, sign):
    case, si = p
    s_lo, s_hi, nband, total = R.case_sums(case, si, sign)
    assert total == sum(R.CASES[case][0] * R.CASES[case][1] * n for n in R.CASES[case][3])
    for pv in R.PV_ALPHAS:
        lo, hi = R.interval(s_lo, s_hi, pv)
        amb = R.caps(lo, hi, nband, total, f"{R.param_id(p)} sign {sign:+d} pv_alpha {pv:.5f}")
        assert (lo <= hi).all()
        print(f"{R.param_id(p)} sign {sign:+d} pv_alpha {pv:.5f}: band {nband} / {total}, ambiguous outputs {amb} / {lo.size}")


def test_the_reference_is_exact_on_the_constructed_cases():
    q, k, v, lengths, alpha, ml = R.uniform_case()
    s_lo, s_hi, nband, total = R.sums(q, k, v, lengths, alpha)
    assert nband == 0 and total > 0 and np.array_equal(s_lo, s_hi) and ml >= max(lengths)
    r = q.shape[1] // k.shape[2]
    assert np.array_equal(s_lo, np.stack([v[b, :n].astype(np.int64).sum(axis=0) for b, n in enumerate(lengths)]).repeat(r, axis=1))
    for i in range(len(R.ONE_HOT)):
        q, k, v, lengths, alpha, ml, hot = R.one_hot_case(i)
        s_lo, s_hi, nband, total = R.sums(q, k, v, lengths, alpha)
        assert nband == 0 and np.array_equal(s_lo, s_hi), R.ONE_HOT[i]
        for pv in (1.0 / 127, 0.003):
            lo, hi = R.interval(s_lo, s_hi, pv)
            assert np.array_equal(lo, hi) and np.array_equal(lo, R.one_hot_expected(v, hot, pv)), R.ONE_HOT[i]
        # the margin the construction promises: the hot key leads every other key of its row by more than 20 / qk_alpha
        hkv, r = k.shape[2], q.shape[1] // k.shape[2]
        for b, n in enumerate(lengths):
            for h in range(q.shape[1]):
                s = k[b, :n, h // r].astype(np.int64) @ q[b, h].astype(np.int64)
                rest = np.delete(s, hot[b, h])
                assert rest.size == 0 or (s[hot[b, h]] - rest.max()) * alpha > 20


def _exact(q, k, v, lengths, alpha, want, what, pvs=(1.0 / 127, 0.003)):
    """the yardstick leaves no room on a constructed case: no P element in the band, s_lo == s_hi, the interval is the one promised value"""
    s_lo, s_hi, nband, total = R.sums(q, k, v, lengths, alpha)
    assert nband == 0 and total > 0 and np.array_equal(s_lo, s_hi), what
    for pv in pvs:
        lo, hi = R.interval(s_lo, s_hi, pv)
        assert np.array_equal(lo, hi) and np.array_equal(lo, want(pv)), what


def _margin(q, k, lengths, alpha, keys, what, least=20):
    """the keys named per (sequence, head) lead every other key of their row by more than `least` / |qk_alpha| (towards the minimum for a negative alpha)"""
    r = q.shape[1] // k.shape[2]
    sign = 1 if alpha > 0 else -1
    for b, n in enumerate(lengths):
        for h in range(q.shape[1]):
            s = sign * (k[b, :n, h // r].astype(np.int64) @ q[b, h].astype(np.int64))
            named = sorted(set(keys(b, h)))
            rest = np.delete(s, named)
            assert rest.size == 0 or (s[named].min() - rest.max()) * abs(alpha) > least, what


def test_one_hot_per_r_and_per_d_is_exact():
    assert [s[1] for s in R.ONE_HOT_R] == list(range(1, 17)) and [s[2] for s in R.ONE_HOT_D] == list(range(16, 257, 16))
    for shapes, make in ((R.ONE_HOT_R, R.one_hot_r_case), (R.ONE_HOT_D, R.one_hot_d_case)):
        for i, shape in enumerate(shapes):
            q, k, v, lengths, alpha, ml, hot = make(i)
            assert list(lengths) == [5, 300] and q.shape[1:] == (shape[0] * shape[1], shape[2])
            _exact(q, k, v, lengths, alpha, lambda pv: R.one_hot_expected(v, hot, pv), shape)
            _margin(q, k, lengths, alpha, lambda b, h: [hot[b, h]], shape)


@pytest.mark.parametrize("nw", [4, 8, 16])
@pytest.mark.parametrize("i", range(len(R.WALK)))
def test_the_key_position_walk_is_exact(i, nw):
    hkv, r, d, tail = R.WALK[i]
    n, C, pos = R.walk_positions(r, nw, tail)
    assert C == R.chunk(r, n + 3) and n == 2 * C + 37 and n % 16 != 0
    want = {C - 65, C - 64, C - 17, C - 16, C - 1, C, C + 1, C + 15, C + 16, C + 63, C + 64, 2 * C - 1, 2 * C, n - 17, n - 16, n - 1}
    if not tail:
        want |= {0, 1, 15, 16, 17, 63, 64, 65, 16 * nw - 1, 16 * nw, 64 * nw - 1, 64 * nw}
    assert set(pos) == want and len(pos) == len(set(pos))
    if nw != 8 and tail:
        return                                                  # the r = 1 positions do not depend on the waves: the same case as at 8
    q, k, v, lengths, alpha, ml, hot = R.walk_case(i, nw)
    assert lengths == (n,) * len(pos) and ml == n + 3 and (hot == np.array(pos)[:, None]).all() and k.shape[1] == ml + 2
    if tail:
        assert (C, n) == (16384, 32805) and k.nbytes < 36 << 20
    _exact(q, k, v, lengths, alpha, lambda pv: R.one_hot_expected(v, hot, pv), R.WALK[i])
    assert np.array_equal(R.one_hot_expected(v, hot, 1.0 / 127), np.stack([v[b, p].repeat(r, axis=0) for b, p in enumerate(pos)]))       # 127 v / 127: v itself
    _margin(q, k, lengths, alpha, lambda b, h: [hot[b, h]], R.WALK[i])


@pytest.mark.parametrize("neg", [False, True], ids=["pos", "neg"])
@pytest.mark.parametrize("i", range(len(R.WALK)))
def test_the_two_weights_are_exact(i, neg):
    hkv, r, d, tail = R.WALK[i]
    q, k, v, lengths, alpha, ml, places = R.two_weight_case(i, neg)
    n = lengths[0]
    C = R.chunk(r, ml)
    assert (alpha < 0) == neg and n > C and (n == 20000) == tail
    assert [(pa // C, pb // C) for pa, pb in places] == [(0, (n - 1) // C), ((n - 1) // C, 0), (0, 1), (1, 0), (1, 1)]
    assert places[2] == (C - 1, C) and places[3] == (C, C - 1)
    _exact(q, k, v, lengths, alpha, lambda pv: R.two_weight_expected(v, places, r, pv), (R.WALK[i], neg))
    _margin(q, k, lengths, alpha, lambda b, h: places[b], (R.WALK[i], neg), least=40)
    for b, (pa, pb) in enumerate(places):                       # A trails B by exactly 400 on every row: one natural unit at qk_alpha = 1 / 400
        sa, sb = (k[b, p, 0].astype(np.int64) @ q[b].astype(np.int64).T for p in (pa, pb))
        assert ((sb - sa) * (-1 if neg else 1) == 400).all() and abs(alpha) == 1.0 / 400
    t = 127 * np.exp([-1.0, 0.0]) / (1 + np.exp(-1.0))
    assert tuple(np.rint(t).astype(int)) == R.TWO_WEIGHTS and (np.abs(t - np.floor(t) - 0.5) > 0.34).all() and R.SR.band_width(20000) * 93 < 0.23


def test_the_poisoned_tail_wins_its_row_outright():
    for case in R.POISONED:
        hkv, r, d, lengths = R.CASES[case]
        q, _, _, _ = R.operands(case)
        k2, v2, k0, v0, kv_len, n_b = R.poisoned(case)
        ml = R.max_len(lengths)
        assert kv_len[0] > ml and n_b[0] == ml and list(n_b[1:]) == list(kv_len[1:]) == list(lengths[1:]) and k2.shape[1] == ml + 2
        for b, n in enumerate(n_b):
            assert np.array_equal(k2[b, :n], k0[b, :n]) and np.array_equal(v2[b, :n], v0[b, :n]) and not k0[b, n:].any() and not v0[b, n:].any()
            assert (np.abs(v2[b, n:]) == 127).all() and n < k2.shape[1]
            for g in range(hkv):
                row = g * r + n % r
                assert k2[b, n, g].astype(np.int64) @ q[b, row].astype(np.int64) == 127 * np.abs(q[b, row].astype(np.int64)).sum()       # the most any key can score
        s_lo, s_hi, nband, total = R.poisoned_sums(case)        # the yardstick's caps at the clamped lengths the GPU test judges by
        amb = R.caps(*R.interval(s_lo, s_hi, R.PV_ALPHAS[0]), nband, total, f"poisoned case {case}")
        print(f"poisoned case {case}: band {nband} / {total}, ambiguous outputs {amb} / {s_lo.size}")


def _model_cases():
    """(name, q, k, v, lengths, qk_alpha, max_len, (s_lo, s_hi), with defects): the constructed chunked cases, and the chunked interval cases (the defects at the middle
    score deviation only: the faithful model is what has to pass everywhere)"""
    for i in range(len(R.WALK) - 1):                            # (the r = 1 shapes run on the device; their rows are no different to the model)
        q, k, v, lengths, alpha, ml, _ = R.walk_case(i)
        yield f"walk {R.WALK[i][:3]}", q, k, v, lengths, alpha, ml, R.sums(q, k, v, lengths, alpha)[:2], True
        for neg in (False, True):
            q, k, v, lengths, alpha, ml, _ = R.two_weight_case(i, neg)
            yield f"two weights {R.WALK[i][:3]} {'-' if neg else '+'}", q, k, v, lengths, alpha, ml, R.sums(q, k, v, lengths, alpha)[:2], True
    for ci in range(len(R.CASES)):
        if R.chunked(ci):
            q, k, v, lengths = R.operands(ci)
            for si in range(len(R.SDS)):
                for sign in (1, -1) if ci >= R.NEW_CASES else (1,):
                    yield f"{R.CASES[ci][:3]} sd {R.SDS[si]:g} {'-' if sign < 0 else '+'}", q, k, v, lengths, sign * R.qk_alpha(ci, si), R.max_len(lengths), R.case_sums(ci, si, sign)[:2], si == 1


def _outside(out, lo, hi):
    out = out.astype(np.int64)
    return int(((out < lo) | (out > hi)).sum())


def test_the_model_passes_and_each_defect_is_caught():
    pv = R.PV_ALPHAS[0]
    caught = {d: [] for d in R.DEFECTS}
    for name, q, k, v, lengths, alpha, ml, s, with_defects in _model_cases():
        lo, hi = R.interval(*s, pv)
        R.check(R.model_out(q, k, v, lengths, alpha, pv, ml), lo, hi, f"the faithful model on {name}")
        for d in R.DEFECTS[:4] if with_defects else ():
            if _outside(R.model_out(q, k, v, lengths, alpha, pv, ml, d), lo, hi):
                caught[d].append(name)
    for case in R.POISONED:
        q = R.operands(case)[0]
        k2, v2, _, _, _, n_b = R.poisoned(case)
        ml, alpha = R.max_len(R.CASES[case][3]), R.qk_alpha(case, 1)
        lo, hi = R.interval(*R.poisoned_sums(case)[:2], pv)
        R.check(R.model_out(q, k2, v2, n_b, alpha, pv, ml), lo, hi, f"the faithful model on the poisoned case {case}")
        if _outside(R.model_out(q, k2, v2, n_b, alpha, pv, ml, "tail_plus_one"), lo, hi):
            caught["tail_plus_one"].append(f"poisoned {case}")
    for d, names in caught.items():
        print(f"{d}: caught on {len(names)} cases: {names}")
    two = [f"two weights {w[:3]} {s}" for w in R.WALK[:-1] for s in "+-"]
    walks = [f"walk {w[:3]}" for w in R.WALK[:-1]]
    # random data shows a missing or stale rescale where a later chunk is long enough to move a row's reference: the cases with a sequence of two full chunks or more
    moving = [f"{shape} sd 4 {s}" for shape in ((1, 16, 256), (1, 8, 128), (2, 4, 128), (1, 12, 64)) for s in "+-"]
    for d, must in (("no_rescale", two + moving), ("stale_reference", two + moving), ("edge_twice", two), ("drop_last_tile", walks),
                    ("tail_plus_one", [f"poisoned {c}" for c in R.POISONED])):
        missed = [n for n in must if n not in caught[d]]
        assert not missed, f"the defect {d} passes on {missed}"

