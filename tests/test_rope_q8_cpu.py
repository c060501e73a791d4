"""CPU: the second C-ABI header (include/asq_hip_attn.h) and its loader table, the argument rules of asq_rope_quantize_qkv in their stated order (NULL and
made-up pointers: nothing is launched), the refusals of ops.rope_quantize_qkv / RopeQuantQKV, and Int8KVCache's bookkeeping.  The same discipline as
tests/test_abi_cpu.py and tests/test_guardband_cpu.py keep for include/asq_hip.h, over the new table."""
import os
import re

import pytest
import torch

from autosmoothquant_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIM, ERR_DTYPE, ERR_ALIGN = 0, -1, -2, -3, -4
F32, F16, BF16 = L.ASQ_F32, L.ASQ_F16, L.ASQ_BF16
ATTN_PURE_QUERIES = set()        # entries of ATTN_SIGNATURES that write no device memory: none so far


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asq_[a-z0-9_]+)\s*\(", src)))


def test_attn_header_and_table_name_the_same_exported_symbols():
    h = L.lib()
    names = _declared("asq_hip_attn.h")
    assert "asq_rope_quantize_qkv" in names
    assert sorted(L.ATTN_SIGNATURES) == names
    for n in names:
        assert hasattr(h, n), f"libasq_hip.so lacks {n}"
        fn = getattr(h, n)
        assert (fn.restype, list(fn.argtypes)) == (L.ATTN_SIGNATURES[n][0], list(L.ATTN_SIGNATURES[n][1]))     # lib() has set it up
    assert not set(L.ATTN_SIGNATURES) & set(L.SIGNATURES)
    assert not set(names) & set(_declared("asq_hip.h"))
    assert h.asq_version() == L.ASQ_VERSION == 126            # the capability probe is the symbol's presence


def test_every_attn_writer_has_a_guard_band_case():
    import test_hip_guardband_rope_q8 as T
    covered = {c.entry for c in T.CASES}
    assert ATTN_PURE_QUERIES <= set(L.ATTN_SIGNATURES) and not (covered & ATTN_PURE_QUERIES)
    assert covered <= set(L.ATTN_SIGNATURES), sorted(covered - set(L.ATTN_SIGNATURES))
    missing = sorted(set(L.ATTN_SIGNATURES) - ATTN_PURE_QUERIES - covered)
    assert not missing, f"entries of include/asq_hip_attn.h without a guard-band case in tests/test_hip_guardband_rope_q8.py: {missing}"
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert covered == empty, sorted(covered - empty)          # every writer also has its "nothing to do" case
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


P, ODD = 1 << 20, (1 << 20) + 8        # made-up device addresses: 16-byte aligned, and not


def _call(dt=F16, B=1, S=2, Hq=2, Hkv=1, D=16, T=8, pos=0, qp=0, kp=0, vp=0, kvb=0, ptrs=None, **named):
    """the raw entry with sane small arguments except those given; ptrs: one value for all eight pointers, named: q / k / v / cos / sin / q8 / k8 / v8 alone"""
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "cos", "sin", "q8", "k8", "v8")}
    p.update(named)
    return L.lib().asq_rope_quantize_qkv(p["q"], p["k"], p["v"], qp, kp, vp, dt, p["cos"], p["sin"], T, pos, p["q8"], p["k8"], p["v8"], kvb, 0.37, 0.11, 0.73,
                                         B, S, Hq, Hkv, D, None)


NULLS, ODDS = [None], [ODD]
BAD_DIMS = [dict(B=-1), dict(S=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(pos=-1), dict(T=-1), dict(S=1 << 31), dict(Hq=1 << 31), dict(D=1 << 20),
            dict(B=(1 << 31) - 1, S=(1 << 31) - 1, Hq=(1 << 31) - 2), dict(B=1 << 20, S=1 << 20, Hq=64, D=128)]
EMPTY = [dict(B=0), dict(S=0), dict(Hq=0), dict(Hkv=0)]
# rule 5, each alone on otherwise valid arguments: (arguments, dtype)
BAD_SHAPE = [(dict(D=24), F16), (dict(D=8), F16), (dict(D=8), BF16), (dict(D=12), F32), (dict(D=4), F32),
             (dict(qp=16), F16), (dict(kp=8), F16), (dict(vp=8), F16),                      # below Hq * D = 32 / Hkv * D = 16
             (dict(qp=36), F16), (dict(kp=20), BF16), (dict(vp=20), F16), (dict(qp=34), F32),    # not a multiple of 8 elements (fp32: 4)
             (dict(kvb=16), F16), (dict(kvb=40), F16),                                      # below S * Hkv * D = 32; not a multiple of 16
             (dict(pos=7), F16), (dict(T=1), F16), (dict(pos=5, T=6), F32)]                 # pos0 + S > tab_rows
# ... and what those rules still accept, seen as the NEXT rule's code on misaligned pointers
GOOD_SHAPE = [(dict(D=8), F32), (dict(qp=36, kp=20, vp=20), F32), (dict(qp=40, kp=48, vp=24), F16), (dict(kvb=32), F16), (dict(kvb=48), BF16), (dict(pos=6), F16),
              (dict(pos=4, T=6), F16)]


def test_argument_errors_come_in_the_stated_order():
    h = L.lib()
    for bad in BAD_DIMS:                                        # 1: dims first -- whatever the dtype and the pointers
        assert _call(**bad) == _call(**bad, dt=7, ptrs=NULLS) == ERR_DIM, bad
        assert b"asq_rope_quantize_qkv" in h.asq_last_error()
    assert _call(dt=7, ptrs=NULLS) == _call(dt=-1, B=0) == _call(dt=3, D=24, ptrs=ODDS) == ERR_DTYPE        # 2: then the dtype, also for an empty problem
    for e in EMPTY:                                             # 3: nothing to do is ASQ_OK whatever the pointers and the rest
        for dt in (F32, F16, BF16):
            assert _call(**e, dt=dt, ptrs=NULLS) == _call(**e, dt=dt, ptrs=ODDS, D=24, qp=3, kvb=5, pos=100) == OK, e
    for name in ("q", "k", "v", "cos", "sin", "q8", "k8", "v8"):                                              # 4: NULL before the shape rules and the alignment
        assert _call(**{name: None}) == _call(**{name: None}, D=24, qp=3, kvb=5, pos=100, ptrs=ODDS) == ERR_NULL, name
    for bad, dt in BAD_SHAPE:                                   # 5: the shape rules before the alignment
        assert _call(**bad, dt=dt) == _call(**bad, dt=dt, ptrs=ODDS) == ERR_DIM, (bad, dt)
    for name in ("q", "k", "v", "cos", "sin", "q8", "k8", "v8"):                                              # 6: every pointer's alignment
        assert _call(**{name: ODD}) == ERR_ALIGN, name
        assert b"16-B aligned" in h.asq_last_error()
    for good, dt in GOOD_SHAPE:
        assert _call(**good, dt=dt, ptrs=ODDS) == ERR_ALIGN, (good, dt)


def _qkv(B=2, S=3, Hq=4, Hkv=2, D=16, dt=torch.float16, T=8):
    z = lambda *s: torch.zeros(s, dtype=dt)  # noqa: E731
    return z(B, S, Hq, D), z(B, S, Hkv, D), z(B, S, Hkv, D), z(T, D // 2), z(T, D // 2)


def test_op_and_module_refuse_cpu_tensors_loudly():
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.nn.attention import Int8KVCache, RopeQuantQKV
    q, k, v, cos, sin = _qkv()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rope_quantize_qkv(q, k, v, cos, sin, 0.37, 0.11, 0.73)
    mod = RopeQuantQKV(0.37, 0.11, 0.73)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(q, k, v, cos, sin, pos=2)
    cache = Int8KVCache(2, 8, 2, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(q, k, v, cos, sin, cache=cache)
    assert cache.length == 0                                    # a refused call does not advance the cache


def test_op_refuses_bad_strides_shapes_and_half_a_cache_slot():
    from autosmoothquant_amd import ops
    q, k, v, cos, sin = _qkv()
    B, S, Hq, Hkv, D = 2, 3, 4, 2, 16
    i8 = lambda *s: torch.zeros(s, dtype=torch.int8)  # noqa: E731
    kc, vc = i8(B, 8, Hkv, D), i8(B, 8, Hkv, D)
    bad = [
        dict(q=q.transpose(1, 2)),                                              # heads before tokens: H * D is not contiguous
        dict(q=torch.zeros(B, S, Hq, 2 * D, dtype=q.dtype)[..., :D]),           # a head's D elements are not followed by the next head
        dict(k=torch.zeros(B, 2 * S + 1, Hkv, D, dtype=q.dtype)[:, :2 * S:2]),  # batch stride is not S row pitches
        dict(v=torch.zeros(S, B, Hkv, D, dtype=q.dtype).transpose(0, 1)),
        dict(q=q[0]), dict(q=q.to(torch.int8)),                                 # not 4-D, not a float dtype
        dict(k=k.float()), dict(v=v[:, :2]), dict(k=k[..., :8]), dict(v=torch.zeros(B, S, 3, D, dtype=q.dtype)),      # k / v disagree with q or with each other
        dict(cos=cos[:, :4]), dict(sin=sin[:2]), dict(cos=cos[:2], sin=sin[:2]), dict(pos=6), dict(pos=-1),           # tables: [T, D/2] with T >= pos + S
        dict(k_out=kc[:, 2:5]), dict(v_out=vc[:, 2:5]),                         # one of the two
        dict(k_out=kc[:, 2:5], v_out=vc[:, 2:4]),                               # not [B, S, Hkv, D]
        dict(k_out=kc[:, 2:5], v_out=vc[:, 2:5].to(torch.int16)),
        dict(k_out=kc[:, 2:5], v_out=i8(B, 16, Hkv, D)[:, 2:5]),                # two batch pitches
        dict(k_out=kc[:, 0:6:2], v_out=vc[:, 0:6:2]),                           # rows of the slot are not consecutive
        dict(k_out=i8(B, 8, Hkv, 2 * D)[:, 2:5, :, :D], v_out=vc[:, 2:5]),
        dict(k_out=i8(S, B, Hkv, D).transpose(0, 1), v_out=i8(S, B, Hkv, D).transpose(0, 1)),      # sequences interleaved token by token
        dict(k_out=i8(1024).as_strided((B, S, Hkv, D), (32, 32, 16, 1)), v_out=i8(1024).as_strided((B, S, Hkv, D), (32, 32, 16, 1))),   # batch pitch below S * Hkv * D
    ]
    for kw in bad:
        args = dict(q=q, k=k, v=v, cos=cos, sin=sin, pos=0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.rope_quantize_qkv(args.pop("q"), args.pop("k"), args.pop("v"), args.pop("cos"), args.pop("sin"), 0.37, 0.11, 0.73, **args)
    # what the stride rule accepts reaches the device check: slices of a fused buffer, a padded pitch, S == 1 with the batch stride as the pitch, a cache slot
    fused = torch.zeros(B, S, (Hq + 2 * Hkv) * D + 8, dtype=q.dtype)
    fq, fk, fv = (fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))
    for args, kw in (((fq, fk, fv), {}), ((fq[:, :1], fk[:, :1], fv[:, :1]), {}), ((q, k, v), dict(k_out=kc[:, 2:5], v_out=vc[:, 2:5], pos=5))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.rope_quantize_qkv(*args, cos, sin, 0.37, 0.11, 0.73, **kw)


def test_module_keeps_three_host_scalars_that_follow_its_dtype():
    from autosmoothquant_amd.layers.nn.attention import RopeQuantQKV
    m = RopeQuantQKV(0.37, 0.11, 0.73)
    assert sorted(m.state_dict()) == ["k_scale", "q_scale", "v_scale"] and all(t.dim() == 0 for t in m.state_dict().values())
    assert m._scales() == tuple(torch.tensor(s).item() for s in (0.37, 0.11, 0.73))
    m.half()
    assert m.q_scale.dtype == torch.float16 and m._scales() == tuple(torch.tensor(s).half().item() for s in (0.37, 0.11, 0.73))
    m2 = RopeQuantQKV()
    m2.load_state_dict(RopeQuantQKV(0.5, 0.25, 2.0).state_dict())
    assert m2._scales() == (0.5, 0.25, 2.0)
    assert all(m2._buffers[n].device.type == "cpu" for n in RopeQuantQKV._SCALES)


def test_int8_kv_cache_bookkeeping():
    from autosmoothquant_amd.layers.nn.attention import Int8KVCache
    c = Int8KVCache(2, 8, 3, 16, device="cpu")
    assert c.k.shape == c.v.shape == (2, 8, 3, 16) and c.k.dtype == c.v.dtype == torch.int8 and c.length == 0 and c.max_len == 8
    assert c.k.data_ptr() != c.v.data_ptr()
    k0, v0 = c.view()
    assert k0.shape == v0.shape == (2, 0, 3, 16)
    ks, vs = c.slot(5)
    assert ks.shape == vs.shape == (2, 5, 3, 16) and ks.stride() == (8 * 48, 48, 16, 1) and c.length == 0     # slot() alone moves nothing
    ks.fill_(7), vs.fill_(-3)                                   # the views alias the buffers
    assert bool((c.k[:, :5] == 7).all()) and bool((c.k[:, 5:] == 0).all()) and bool((c.v[:, :5] == -3).all()) and bool((c.v[:, 5:] == 0).all())
    c.advance(5)
    assert c.length == 5
    kv, vv = c.view()
    assert kv.shape == (2, 5, 3, 16) and kv.data_ptr() == c.k.data_ptr() and vv.data_ptr() == c.v.data_ptr() and bool((kv == 7).all()) and bool((vv == -3).all())
    k1, v1 = c.slot(1)
    assert k1.data_ptr() == c.k.data_ptr() + 5 * 48 and v1.data_ptr() == c.v.data_ptr() + 5 * 48 and k1.shape == (2, 1, 3, 16)
    c.advance(1)
    c.slot(2), c.advance(2)
    assert c.length == 8 and c.slot(0)[0].shape == (2, 0, 3, 16)
    for call in (lambda: c.slot(1), lambda: c.advance(1), lambda: c.slot(-1)):
        with pytest.raises(ValueError):
            call()
    assert c.length == 8
    c.reset()
    assert c.length == 0 and c.view()[0].shape == (2, 0, 3, 16) and c.slot(8)[0].shape == (2, 8, 3, 16)
    assert bool((c.k[:, :5] == 7).all())                        # reset() forgets, it does not clear
    one = Int8KVCache(1, 8, 3, 16)
    one.advance(4)
    assert all(t.is_contiguous() for t in one.view())           # a single sequence's prefix is contiguous: what Int8Attention(layout="bshd") takes as it is
