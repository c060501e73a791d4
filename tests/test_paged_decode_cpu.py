"""CPU: the fourth C-ABI header (include/asq_hip_paged.h) and its loader table with the discipline tests/test_attn_decode_cpu.py keeps over the third, the argument
rules of asq_attn_decode_i8_paged and asq_rope_quantize_qkv_paged in their stated order (NULL and made-up pointers: nothing is launched), the refusals of the ops
and the modules, and PagedInt8KVCache's bookkeeping on device="cpu"."""
import os
import re

import pytest
import torch

from autosmoothquant_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIM, ERR_DTYPE, ERR_ALIGN = 0, -1, -2, -3, -4
F32, F16, BF16 = L.ASQ_F32, L.ASQ_F16, L.ASQ_BF16
PAGED_PURE_QUERIES = set()       # entries of PAGED_SIGNATURES that write no device memory: none
P, ODD, ODD4 = 1 << 20, (1 << 20) + 8, (1 << 20) + 2        # made-up device addresses: 16-byte aligned, 8-byte only, 2-byte only


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asq_[a-z0-9_]+)\s*\(", src)))


def test_paged_header_and_table_name_the_same_exported_symbols():
    h = L.lib()
    names = _declared("asq_hip_paged.h")
    assert names == ["asq_attn_decode_i8_paged", "asq_rope_quantize_qkv_paged"]
    assert sorted(L.PAGED_SIGNATURES) == names
    for n in names:
        assert hasattr(h, n), f"libasq_hip.so lacks {n}"
        fn = getattr(h, n)
        assert (fn.restype, list(fn.argtypes)) == (L.PAGED_SIGNATURES[n][0], list(L.PAGED_SIGNATURES[n][1]))       # lib() has set it up
    others = set(L.SIGNATURES) | set(L.ATTN_SIGNATURES) | set(L.DECODE_SIGNATURES)
    assert not set(L.PAGED_SIGNATURES) & others
    assert not set(names) & (set(_declared("asq_hip.h")) | set(_declared("asq_hip_attn.h")) | set(_declared("asq_hip_decode.h")))
    assert h.asq_version() == L.ASQ_VERSION == 126            # the capability probe is the symbol's presence
    mk = open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", "Makefile")).read()
    assert "asq_hip_paged.h" in mk


def test_every_paged_writer_has_a_guard_band_case():
    import test_hip_guardband_paged as T
    covered = {c.entry for c in T.CASES}
    assert PAGED_PURE_QUERIES <= set(L.PAGED_SIGNATURES) and not (covered & PAGED_PURE_QUERIES)
    assert covered <= set(L.PAGED_SIGNATURES), sorted(covered - set(L.PAGED_SIGNATURES))
    missing = sorted(set(L.PAGED_SIGNATURES) - PAGED_PURE_QUERIES - covered)
    assert not missing, f"entries of include/asq_hip_paged.h without a guard-band case in tests/test_hip_guardband_paged.py: {missing}"
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert covered == empty, sorted(covered - empty)          # every writer also has its "nothing to do" case
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def _dec(B=2, Hq=4, Hkv=2, D=16, np_=4, ps=16, pp=0, tp=2, ml=8, ptrs=None, kv_len=P, tab=P, **named):
    """asq_attn_decode_i8_paged with sane small arguments except those given; ptrs: one value for q / k / v / out, named: one of them alone"""
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "out")}
    p.update(named)
    return L.lib().asq_attn_decode_i8_paged(p["q"], p["k"], p["v"], tab, kv_len, p["out"], B, Hq, Hkv, D, np_, ps, pp, tp, ml, 0.01, 0.02, None)


def test_paged_decode_argument_errors_come_in_the_stated_order():
    h = L.lib()
    bad_dims = [dict(B=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(D=257), dict(D=272), dict(ml=-1), dict(ml=1 << 17), dict(B=1 << 31), dict(Hq=1 << 31),
                dict(B=(1 << 31) - 1, Hkv=(1 << 31) - 1, Hq=(1 << 31) - 1), dict(np_=-1), dict(ps=-16), dict(tp=-1), dict(np_=1 << 31), dict(ps=1 << 31), dict(tp=1 << 31),
                dict(ps=(1 << 31) - 16, Hkv=(1 << 31) - 2, Hq=(1 << 31) - 2, D=256)]
    for bad in bad_dims:                                        # 1: dims first, whatever the pointers
        assert _dec(**bad) == _dec(**bad, ptrs=[None], tab=None) == ERR_DIM, bad
        assert b"asq_attn_decode_i8_paged" in h.asq_last_error()
    for e in (dict(B=0), dict(Hq=0), dict(Hkv=0), dict(Hq=0, Hkv=0)):                                            # 2: nothing to do
        assert _dec(**e, ptrs=[None], tab=None) == _dec(**e, ptrs=[ODD], D=24, ps=5, pp=5, kv_len=ODD4, tab=ODD4) == OK, e
    for name in ("q", "k", "v", "out"):                         # 3: NULL before the shape rules and the alignment; kv_len may be NULL, the table may not
        assert _dec(**{name: None}) == _dec(**{name: None}, D=24, ps=5, ptrs=[ODD]) == ERR_NULL, name
    assert _dec(tab=None) == _dec(tab=None, D=24, pp=5, ptrs=[ODD], kv_len=ODD4) == ERR_NULL
    assert _dec(kv_len=None, ptrs=[ODD]) == ERR_ALIGN
    page = 16 * 2 * 16
    bad_shape = [dict(D=24), dict(D=8), dict(Hq=5), dict(Hq=3, Hkv=2), dict(Hq=34, Hkv=2), dict(Hq=17, Hkv=1),
                 dict(ps=0), dict(ps=8), dict(ps=24), dict(ps=17), dict(pp=16), dict(pp=page - 16), dict(pp=page + 8), dict(pp=-16),          # the page size, the page pitch
                 dict(ml=33), dict(tp=0), dict(ps=32, tp=1, ml=33), dict(np_=0), dict(np_=0, ml=1)]          # the table is too narrow for max_len; keys without a pool
    for bad in bad_shape:                                       # 4: the shape rules before the alignment
        assert _dec(**bad) == _dec(**bad, ptrs=[ODD], kv_len=ODD4, tab=ODD4) == ERR_DIM, bad
    for name in ("q", "k", "v", "out"):                         # 5: alignment, 16 B for the tensors and 4 B for kv_len and the table
        assert _dec(**{name: ODD}) == ERR_ALIGN, name
    assert _dec(kv_len=ODD4) == ERR_ALIGN and b"kv_len" in h.asq_last_error()
    assert _dec(tab=ODD4) == ERR_ALIGN and b"block_table" in h.asq_last_error()
    for good in (dict(Hq=32, Hkv=2), dict(Hq=16, Hkv=1), dict(D=256), dict(pp=page), dict(pp=page + 16), dict(ps=16), dict(ps=48, tp=1, ml=48), dict(ml=32), dict(ml=0),
                 dict(ml=0, np_=0), dict(ml=0, tp=0), dict(ml=(1 << 17) - 1, tp=1 << 13), dict(kv_len=None), dict(kv_len=P + 4), dict(tab=P + 4), dict(np_=1)):
        assert _dec(**good, out=ODD) == ERR_ALIGN, good            # accepted by rules 1 - 4: seen as the next rule's code


def _app(dt=F16, B=1, S=2, Hq=2, Hkv=1, D=16, T=8, qp=0, kp=0, vp=0, np_=4, ps=16, pp=0, tp=2, ml=8, ptrs=None, pos=P, tab=P, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "cos", "sin", "q8", "kc", "vc")}
    p.update(named)
    return L.lib().asq_rope_quantize_qkv_paged(p["q"], p["k"], p["v"], qp, kp, vp, dt, p["cos"], p["sin"], T, pos, tab, p["q8"], p["kc"], p["vc"], np_, ps, pp, tp, ml,
                                               0.37, 0.11, 0.73, B, S, Hq, Hkv, D, None)


def test_paged_append_argument_errors_come_in_the_stated_order():
    h = L.lib()
    names = ("q", "k", "v", "cos", "sin", "q8", "kc", "vc")
    bad_dims = [dict(B=-1), dict(S=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(T=-1), dict(ml=-1), dict(ml=1 << 31), dict(S=1 << 31), dict(Hq=1 << 31),
                dict(D=1 << 20), dict(B=(1 << 31) - 1, S=(1 << 31) - 1, Hq=(1 << 31) - 2), dict(B=1 << 20, S=1 << 20, Hq=64, D=128),
                dict(np_=-1), dict(ps=-16), dict(tp=-1), dict(np_=1 << 31), dict(ps=1 << 31), dict(tp=1 << 31)]
    for bad in bad_dims:                                        # 1: dims first -- whatever the dtype and the pointers
        assert _app(**bad) == _app(**bad, dt=7, ptrs=[None], pos=None, tab=None) == ERR_DIM, bad
        assert b"asq_rope_quantize_qkv_paged" in h.asq_last_error()
    assert _app(dt=7, ptrs=[None]) == _app(dt=-1, B=0) == _app(dt=3, D=24, ps=5, ptrs=[ODD]) == ERR_DTYPE          # 2: then the dtype, also for an empty problem
    for e in (dict(B=0), dict(S=0), dict(Hq=0), dict(Hkv=0)):                                            # 3: nothing to do
        for dt in (F32, F16, BF16):
            assert _app(**e, dt=dt, ptrs=[None], pos=None, tab=None) == _app(**e, dt=dt, ptrs=[ODD], D=24, qp=3, ps=5, pp=5, pos=ODD4, tab=ODD4) == OK, e
    for name in names:                                          # 4: NULL, pos and the table included, before the shape rules and the alignment
        assert _app(**{name: None}) == _app(**{name: None}, D=24, qp=3, ps=5, ptrs=[ODD]) == ERR_NULL, name
    assert _app(pos=None) == _app(pos=None, D=24, ptrs=[ODD]) == ERR_NULL
    assert _app(tab=None) == _app(tab=None, ps=24, ptrs=[ODD], pos=ODD4) == ERR_NULL
    page = 16 * 16
    bad_shape = [(dict(D=24), F16), (dict(D=8), BF16), (dict(D=12), F32), (dict(qp=16), F16), (dict(kp=8), F16), (dict(vp=8), F16), (dict(qp=36), F16), (dict(qp=34), F32),
                 (dict(ps=0), F16), (dict(ps=8), F16), (dict(ps=24), BF16), (dict(pp=16), F16), (dict(pp=page - 16), F16), (dict(pp=page + 8), F16), (dict(pp=-16), F32),
                 (dict(ml=33), F16), (dict(tp=0), F16), (dict(np_=0), F16)]
    for bad, dt in bad_shape:                                   # 5: the shape rules before the alignment
        assert _app(**bad, dt=dt) == _app(**bad, dt=dt, ptrs=[ODD], pos=ODD4, tab=ODD4) == ERR_DIM, (bad, dt)
    for name in names:                                          # 6: every pointer's alignment, 4 B for pos and the table
        assert _app(**{name: ODD}) == ERR_ALIGN, name
    assert _app(pos=ODD4) == ERR_ALIGN and b"pos" in h.asq_last_error()
    assert _app(tab=ODD4) == ERR_ALIGN and b"block_table" in h.asq_last_error()
    for good, dt in [(dict(D=8), F32), (dict(pp=page), F16), (dict(pp=page + 16), F16), (dict(ps=16), F16), (dict(ps=48, tp=1, ml=48), F16), (dict(ml=32), F16),
                     (dict(T=0), F16), (dict(T=1), F16), (dict(ml=0), F16), (dict(ml=0, np_=0, tp=0), F16), (dict(pos=P + 4), BF16), (dict(tab=P + 4), BF16)]:
        assert _app(**good, dt=dt, ptrs=[ODD]) == ERR_ALIGN, (good, dt)          # positions and page ids are the device's business: no host rule


def _i8(*s):
    return torch.zeros(s, dtype=torch.int8)


def test_paged_ops_and_modules_refuse_cpu_tensors_bad_strides_and_mismatched_pools():
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, PagedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, NP, PS, TW = 2, 4, 2, 16, 6, 16, 3
    q, kp, vp = _i8(B, Hq, D), _i8(NP, PS, Hkv, D), _i8(NP, PS, Hkv, D)
    n, tab = torch.zeros(B, dtype=torch.int32), torch.zeros((B, TW), dtype=torch.int32)
    wide = torch.zeros((B, TW + 2), dtype=torch.int32)
    for args, kw in (((q, kp, vp, tab, n), {}), ((q.view(B, 1, Hq, D), kp, vp, wide[:, :TW], None), {}), ((q, kp, vp, tab, n), dict(max_len=3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.attn_decode_i8_paged(*args, 0.01, 0.02, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Int8Attention(0.01, 0.02).decode_paged(q.view(B, 1, Hq, D), kp, vp, tab, n)
    bad = [
        dict(q=q.float()), dict(q=q[0]), dict(q=_i8(B, 2, Hq, D)), dict(q=_i8(B, Hq, 2 * D)[..., :D]), dict(q=_i8(B + 1, Hq, D)),
        dict(q=_i8(B, 34, D)), dict(q=_i8(B, 5, D)),            # r = 17; Hq no multiple of Hkv
        dict(q=_i8(B, Hq, 24), k_pool=_i8(NP, PS, Hkv, 24), v_pool=_i8(NP, PS, Hkv, 24)),      # D no multiple of 16
        dict(k_pool=kp.transpose(1, 2)), dict(k_pool=kp[:, ::2], v_pool=vp[:, ::2]), dict(k_pool=_i8(NP, PS, Hkv, 2 * D)[..., :D]),
        dict(k_pool=_i8(NP, 24, Hkv, D), v_pool=_i8(NP, 24, Hkv, D)),                          # a page size that is no multiple of 16
        dict(k_pool=kp[:, :8], v_pool=vp[:, :8]),
        dict(k_pool=kp[:4]),                                    # the two pools disagree
        dict(v_pool=_i8(NP, 2 * PS, Hkv, D)[:, :PS]),           # two page pitches
        dict(v_pool=vp.to(torch.int16)), dict(k_pool=kp[0], v_pool=vp[0]),
        dict(block_table=tab.long()), dict(block_table=tab[0]), dict(block_table=torch.zeros((B + 1, TW), dtype=torch.int32)), dict(block_table=[[0, 1, 2]] * B),
        dict(block_table=wide[:, ::2]), dict(block_table=torch.zeros((TW, B), dtype=torch.int32).t()),
        dict(kv_len=n.long()), dict(kv_len=torch.zeros(B + 1, dtype=torch.int32)), dict(kv_len=[1, 2]),
        dict(max_len=TW * PS + 1), dict(max_len=-1),
    ]
    for kw in bad:
        a = dict(q=q, k_pool=kp, v_pool=vp, block_table=tab, kv_len=n, max_len=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_decode_i8_paged(a["q"], a["k_pool"], a["v_pool"], a["block_table"], a["kv_len"], 0.01, 0.02, max_len=a["max_len"])
    with pytest.raises(ValueError):
        Int8Attention(0.01, 0.02).decode_paged(q, kp, vp, tab, n)          # the module takes [B, 1, Hq, d]
    # the append: rope_quantize_qkv_at's rules, two pools of one shape and pitch, an int32 [B, T] table
    z = lambda *s: torch.zeros(s, dtype=torch.float16)  # noqa: E731
    S, T = 3, 8
    fq, fk, fv, cos, sin = z(B, S, Hq, D), z(B, S, Hkv, D), z(B, S, Hkv, D), z(T, D // 2), z(T, D // 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rope_quantize_qkv_paged(fq, fk, fv, cos, sin, 0.37, 0.11, 0.73, n, tab, kp, vp)
    for kw in (dict(q=fq.transpose(1, 2)), dict(k=fk.float()), dict(v=fv[:, :2]), dict(cos=cos[:, :4]), dict(pos=n.long()), dict(pos=torch.zeros(3, dtype=torch.int32)),
               dict(pos=0), dict(k_pool=kp[:4]), dict(k_pool=kp[:, ::2], v_pool=vp[:, ::2]), dict(v_pool=_i8(NP, PS, Hkv + 1, D)), dict(k_pool=kp[:, :8], v_pool=vp[:, :8]),
               dict(block_table=tab.long()), dict(block_table=tab[:1]), dict(block_table=wide[:, ::2]), dict(max_len=TW * PS + 1)):
        a = dict(q=fq, k=fk, v=fv, cos=cos, sin=sin, pos=n, block_table=tab, k_pool=kp, v_pool=vp, max_len=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.rope_quantize_qkv_paged(a["q"], a["k"], a["v"], a["cos"], a["sin"], 0.37, 0.11, 0.73, a["pos"], a["block_table"], a["k_pool"], a["v_pool"], max_len=a["max_len"])
    mod, cache = RopeQuantQKV(0.37, 0.11, 0.73), PagedInt8KVCache(NP, PS, Hkv, D, B, 40, device="cpu")
    state = lambda: (list(cache.lengths), [list(p) for p in cache.pages], list(cache.free), cache.kv_len.tolist(), cache.block_table.tolist())  # noqa: E731
    cache.reserve([30, 0])
    cache.advance([30, 0])
    before = state()
    with pytest.raises(ValueError):
        mod(fq, fk, fv, cos, sin, cache=cache, advance=[4, 1])                 # more than the 3 rows written
    with pytest.raises(ValueError):
        mod(z(B, 11, Hq, D), z(B, 11, Hkv, D), z(B, 11, Hkv, D), cos, sin, cache=cache)          # 30 + 11 > max_len 40: refused before anything is launched
    assert state() == before
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(fq, fk, fv, cos, sin, cache=cache)                  # 3 rows that would take sequence 1's first page: the refused append keeps no page
    assert state()[:4] == before[:4]
    assert sorted(Int8Attention(0.01, 0.02).state_dict()) == ["pv_bmm.a", "qk_bmm.a"]          # decode_paged() adds no state


def test_paged_cache_bookkeeping():
    from autosmoothquant_amd.layers.nn.attention import PagedInt8KVCache
    NP, PS, Hkv, D, B, ML = 7, 16, 2, 16, 3, 70
    c = PagedInt8KVCache(NP, PS, Hkv, D, B, ML, device="cpu")
    assert c.k.shape == c.v.shape == (NP, PS, Hkv, D) and c.k.dtype == c.v.dtype == torch.int8 and c.k.data_ptr() != c.v.data_ptr() and c.page_size == PS and c.max_len == ML
    assert c.block_table.shape == (B, 5) and c.block_table.dtype == c.kv_len.dtype == torch.int32 and c.kv_len.tolist() == c.lengths == [0, 0, 0] and c.bound() == 0
    ptrs = (c.block_table.data_ptr(), c.kv_len.data_ptr())
    state = lambda: (list(c.lengths), [list(p) for p in c.pages], sorted(c.free), c.kv_len.tolist(), c.block_table.tolist())  # noqa: E731
    c.reserve([15, 0, 1])
    assert [len(p) for p in c.pages] == [1, 0, 1] and len(c.free) == NP - 2 and c.lengths == [0, 0, 0]          # reserve() does not advance
    c.advance([15, 0, 1])
    assert c.kv_len.tolist() == c.lengths == [15, 0, 1] and c.bound() == 15
    c.reserve(1)                                                # sequence 0 fills its page, sequence 1 takes its first, sequence 2 stays inside its own
    assert [len(p) for p in c.pages] == [1, 1, 1]
    c.advance(1)
    c.reserve([1, 0, 0])                                        # across the page edge: exactly one page
    assert [len(p) for p in c.pages] == [2, 1, 1] and len(c.free) == NP - 4
    c.advance([1, 0, 0])
    assert c.lengths == [17, 1, 2]
    for b in range(B):                                          # the table's used entries are the host's page lists, all distinct
        assert c.block_table[b, :len(c.pages[b])].tolist() == c.pages[b]
    held = [p for pg in c.pages for p in pg]
    assert len(set(held)) == len(held) and sorted(held + c.free) == list(range(NP))
    before = state()
    for bad in (lambda: c.reserve([0, 16 * 4, 0]),              # 4 more pages, 3 are free
                lambda: c.reserve([54, 0, 0]),                  # 17 + 54 > max_len
                lambda: c.reserve([1, 1]), lambda: c.reserve(-1), lambda: c.reserve([0, 0, -1]),
                lambda: c.advance([16, 0, 0]),                  # beyond the reserved pages
                lambda: c.advance([0, 0, 69]), lambda: c.advance(-1)):
        with pytest.raises(ValueError):
            bad()
        assert state() == before                                # a refused call moves nothing
    own = list(c.pages[0])
    free_before = list(c.free)
    c.reset(0)
    assert c.lengths == [0, 1, 2] and c.kv_len.tolist() == [0, 1, 2] and c.pages[0] == [] and sorted(c.free) == sorted(free_before + own)       # exactly that sequence's pages
    c.reserve([0, 32, 0])
    assert c.pages[1][1:] == own                              # freed pages are reused, the freed sequence's first page first
    c.k.fill_(7)
    c.reset(-1)
    assert c.lengths == [0, 1, 0]
    c.reset()
    assert c.kv_len.tolist() == c.lengths == [0, 0, 0] and sorted(c.free) == list(range(NP)) and bool((c.k == 7).all())          # reset() forgets, it does not clear
    assert (c.block_table.data_ptr(), c.kv_len.data_ptr()) == ptrs             # what a captured step reads stays where it is
    # gather round-trips rows written by hand
    c.reserve([20, 0, 33])
    c.advance([20, 0, 33])
    g = torch.Generator().manual_seed(52720)
    want = {}
    for b in (0, 2):
        n = c.lengths[b]
        kk, vv = (torch.randint(-128, 128, (n, Hkv, D), dtype=torch.int8, generator=g) for _ in range(2))
        for i in range(n):
            page = int(c.block_table[b, i // PS])
            c.k[page, i % PS], c.v[page, i % PS] = kk[i], vv[i]
        want[b] = (kk, vv)
    for b in (0, 2):
        gk, gv = c.gather(b)
        assert gk.is_contiguous() and torch.equal(gk, want[b][0]) and torch.equal(gv, want[b][1])
    gk, gv = c.gather(1)
    assert gk.shape == gv.shape == (0, Hkv, D)
    assert (c.block_table.data_ptr(), c.kv_len.data_ptr()) == ptrs
