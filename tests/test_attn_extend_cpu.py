"""CPU: the fifth C-ABI header (include/asq_hip_extend.h) and its loader table with the discipline tests/test_paged_decode_cpu.py keeps over the fourth, the argument
rules of asq_attn_extend_i8 and asq_attn_extend_i8_paged in their stated order (NULL and made-up pointers: nothing is launched), the refusals of the ops and the
modules, rewind() on both caches with device="cpu", and the yardstick of the GPU tests: tests/attn_extend_ref.py's case table keeps attn_decode_ref's caps on the
row-expanded problem for every case, spread and sign, covers the kernel forms it promises, and its intervals collapse to the promised values on the two staircases."""
import os
import re

import numpy as np
import pytest
import torch

import attn_decode_ref as R
import attn_extend_ref as X
from autosmoothquant_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_NULL, ERR_DIM, ERR_DTYPE, ERR_ALIGN = 0, -1, -2, -3, -4
EXTEND_PURE_QUERIES = set()      # entries of EXTEND_SIGNATURES that write no device memory: none
P, ODD, ODD4 = 1 << 20, (1 << 20) + 8, (1 << 20) + 2        # made-up device addresses: 16-byte aligned, 8-byte only, 2-byte only
HEADERS = ("asq_hip.h", "asq_hip_attn.h", "asq_hip_decode.h", "asq_hip_paged.h")


def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(asq_[a-z0-9_]+)\s*\(", src)))


def test_extend_header_and_table_name_the_same_exported_symbols():
    h = L.lib()
    names = _declared("asq_hip_extend.h")
    assert names == ["asq_attn_extend_i8", "asq_attn_extend_i8_paged"]
    assert sorted(L.EXTEND_SIGNATURES) == names
    for n in names:
        assert hasattr(h, n), f"libasq_hip.so lacks {n}"
        fn = getattr(h, n)
        assert (fn.restype, list(fn.argtypes)) == (L.EXTEND_SIGNATURES[n][0], list(L.EXTEND_SIGNATURES[n][1]))       # lib() has set it up
    others = set(L.SIGNATURES) | set(L.ATTN_SIGNATURES) | set(L.DECODE_SIGNATURES) | set(L.PAGED_SIGNATURES)
    assert not set(L.EXTEND_SIGNATURES) & others
    assert not set(names) & set().union(*(_declared(hd) for hd in HEADERS))
    assert h.asq_version() == L.ASQ_VERSION == 126            # the capability probe is the symbol's presence
    mk = open(os.path.join(ROOT, "autosmoothquant_amd", "csrc", "Makefile")).read()
    assert mk.count("asq_hip_extend.h") == 2                  # the header comment and HDRS


def test_every_extend_writer_has_a_guard_band_case():
    import test_hip_guardband_extend as T
    covered = {c.entry for c in T.CASES}
    assert EXTEND_PURE_QUERIES <= set(L.EXTEND_SIGNATURES) and not (covered & EXTEND_PURE_QUERIES)
    assert covered <= set(L.EXTEND_SIGNATURES), sorted(covered - set(L.EXTEND_SIGNATURES))
    missing = sorted(set(L.EXTEND_SIGNATURES) - EXTEND_PURE_QUERIES - covered)
    assert not missing, f"entries of include/asq_hip_extend.h without a guard-band case in tests/test_hip_guardband_extend.py: {missing}"
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert covered == empty, sorted(covered - empty)          # every writer also has its "nothing to do" case
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))


def _ext(B=2, Sq=3, Hq=4, Hkv=2, D=16, pitch=0, ml=8, ptrs=None, kv_len=P, q_len=P, **named):
    """asq_attn_extend_i8 with sane small arguments except those given; ptrs: one value for q / k / v / out, named: one of them alone"""
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "out")}
    p.update(named)
    return L.lib().asq_attn_extend_i8(p["q"], p["k"], p["v"], kv_len, q_len, p["out"], B, Sq, Hq, Hkv, D, pitch, ml, 0.01, 0.02, None)


def test_extend_argument_errors_come_in_the_stated_order():
    h = L.lib()
    bad_dims = [dict(B=-1), dict(Sq=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(D=257), dict(D=272), dict(ml=-1), dict(ml=1 << 17), dict(B=1 << 31),
                dict(Sq=1 << 31), dict(Hq=1 << 31), dict(B=(1 << 31) - 1, Hkv=(1 << 31) - 1, Hq=(1 << 31) - 1), dict(B=1 << 20, Sq=(1 << 31) - 1, Hq=1 << 20, Hkv=1, D=256)]
    for bad in bad_dims:                                        # 1: dims first, whatever the pointers
        assert _ext(**bad) == _ext(**bad, ptrs=[None]) == ERR_DIM, bad
        assert b"asq_attn_extend_i8" in h.asq_last_error()
    for e in (dict(B=0), dict(Sq=0), dict(Hq=0), dict(Hkv=0), dict(Hq=0, Hkv=0)):                              # 2: nothing to do
        assert _ext(**e, ptrs=[None]) == _ext(**e, ptrs=[ODD], D=24, pitch=5, kv_len=ODD4, q_len=ODD4) == OK, e
    for name in ("q", "k", "v", "out"):                         # 3: NULL before the shape rules and the alignment; kv_len and q_len may be NULL
        assert _ext(**{name: None}) == _ext(**{name: None}, D=24, pitch=5, ptrs=[ODD]) == ERR_NULL, name
    assert _ext(kv_len=None, q_len=None, ptrs=[ODD]) == ERR_ALIGN
    bad_shape = [dict(D=24), dict(D=8), dict(Hq=5), dict(Hq=3, Hkv=2), dict(Hq=34, Hkv=2), dict(Hq=17, Hkv=1),
                 dict(B=1 << 10, Hq=1 << 12, Hkv=1 << 8, Sq=1 << 13, ml=0),     # r = 16: one token per workgroup, 2^10 x 2^8 x 2^13 of them
                 dict(pitch=16), dict(pitch=8 * 2 * 16 - 16), dict(pitch=8 * 2 * 16 + 8), dict(pitch=-16)]          # below max_len * Hkv * D = 256; no multiple of 16
    for bad in bad_shape:                                       # 4: the shape rules before the alignment
        assert _ext(**bad) == _ext(**bad, ptrs=[ODD], kv_len=ODD4, q_len=ODD4) == ERR_DIM, bad
    for name in ("q", "k", "v", "out"):                         # 5: alignment, 16 B for the tensors and 4 B for kv_len and q_len
        assert _ext(**{name: ODD}) == ERR_ALIGN, name
    assert _ext(kv_len=ODD4) == ERR_ALIGN and b"kv_len" in h.asq_last_error()
    assert _ext(q_len=ODD4) == ERR_ALIGN and b"q_len" in h.asq_last_error()
    for good in (dict(Hq=32, Hkv=2), dict(Hq=16, Hkv=1), dict(D=256), dict(pitch=256), dict(pitch=272), dict(ml=0), dict(ml=(1 << 17) - 1), dict(kv_len=None), dict(q_len=None),
                 dict(kv_len=P + 4, q_len=P + 8), dict(Sq=1), dict(Sq=100), dict(B=1 << 10, Hq=1 << 12, Hkv=1 << 8, Sq=(1 << 13) - 1, ml=0)):
        assert _ext(**good, out=ODD) == ERR_ALIGN, good            # accepted by rules 1 - 4: seen as the next rule's code


def _extp(B=2, Sq=3, Hq=4, Hkv=2, D=16, np_=4, ps=16, pp=0, tp=2, ml=8, ptrs=None, kv_len=P, q_len=P, tab=P, **named):
    p = {n: (P if ptrs is None else ptrs[0]) for n in ("q", "k", "v", "out")}
    p.update(named)
    return L.lib().asq_attn_extend_i8_paged(p["q"], p["k"], p["v"], tab, kv_len, q_len, p["out"], B, Sq, Hq, Hkv, D, np_, ps, pp, tp, ml, 0.01, 0.02, None)


def test_paged_extend_argument_errors_come_in_the_stated_order():
    h = L.lib()
    bad_dims = [dict(B=-1), dict(Sq=-1), dict(Hq=-1), dict(Hkv=-1), dict(D=0), dict(D=-16), dict(D=257), dict(D=272), dict(ml=-1), dict(ml=1 << 17), dict(B=1 << 31),
                dict(Sq=1 << 31), dict(Hq=1 << 31), dict(B=(1 << 31) - 1, Hkv=(1 << 31) - 1, Hq=(1 << 31) - 1), dict(B=1 << 20, Sq=(1 << 31) - 1, Hq=1 << 20, Hkv=1, D=256),
                dict(np_=-1), dict(ps=-16), dict(tp=-1), dict(np_=1 << 31), dict(ps=1 << 31), dict(tp=1 << 31), dict(ps=(1 << 31) - 16, Hkv=(1 << 31) - 2, Hq=(1 << 31) - 2, D=256)]
    for bad in bad_dims:                                        # 1: dims first, whatever the pointers
        assert _extp(**bad) == _extp(**bad, ptrs=[None], tab=None) == ERR_DIM, bad
        assert b"asq_attn_extend_i8_paged" in h.asq_last_error()
    for e in (dict(B=0), dict(Sq=0), dict(Hq=0), dict(Hkv=0), dict(Hq=0, Hkv=0)):                              # 2: nothing to do
        assert _extp(**e, ptrs=[None], tab=None) == _extp(**e, ptrs=[ODD], D=24, ps=5, pp=5, kv_len=ODD4, q_len=ODD4, tab=ODD4) == OK, e
    for name in ("q", "k", "v", "out"):                         # 3: NULL before the shape rules and the alignment; kv_len and q_len may be NULL, the table may not
        assert _extp(**{name: None}) == _extp(**{name: None}, D=24, ps=5, ptrs=[ODD]) == ERR_NULL, name
    assert _extp(tab=None) == _extp(tab=None, D=24, pp=5, ptrs=[ODD], kv_len=ODD4) == ERR_NULL
    assert _extp(kv_len=None, q_len=None, ptrs=[ODD]) == ERR_ALIGN
    page = 16 * 2 * 16
    bad_shape = [dict(D=24), dict(D=8), dict(Hq=5), dict(Hq=3, Hkv=2), dict(Hq=34, Hkv=2), dict(Hq=17, Hkv=1),
                 dict(B=1 << 10, Hq=1 << 12, Hkv=1 << 8, Sq=1 << 13, ml=0),     # 2^31 workgroups
                 dict(ps=0), dict(ps=8), dict(ps=24), dict(ps=17), dict(pp=16), dict(pp=page - 16), dict(pp=page + 8), dict(pp=-16),          # the page size, the page pitch
                 dict(ml=33), dict(tp=0), dict(ps=32, tp=1, ml=33), dict(np_=0), dict(np_=0, ml=1)]          # the table is too narrow for max_len; keys without a pool
    for bad in bad_shape:                                       # 4: the shape rules before the alignment
        assert _extp(**bad) == _extp(**bad, ptrs=[ODD], kv_len=ODD4, q_len=ODD4, tab=ODD4) == ERR_DIM, bad
    for name in ("q", "k", "v", "out"):                         # 5: alignment, 16 B for the tensors and 4 B for kv_len, q_len and the table
        assert _extp(**{name: ODD}) == ERR_ALIGN, name
    assert _extp(kv_len=ODD4) == ERR_ALIGN and b"kv_len" in h.asq_last_error()
    assert _extp(q_len=ODD4) == ERR_ALIGN and b"q_len" in h.asq_last_error()
    assert _extp(tab=ODD4) == ERR_ALIGN and b"block_table" in h.asq_last_error()
    for good in (dict(Hq=32, Hkv=2), dict(Hq=16, Hkv=1), dict(D=256), dict(pp=page), dict(pp=page + 16), dict(ps=48, tp=1, ml=48), dict(ml=32), dict(ml=0),
                 dict(ml=0, np_=0), dict(ml=0, tp=0), dict(ml=(1 << 17) - 1, tp=1 << 13), dict(kv_len=None), dict(q_len=None), dict(tab=P + 4), dict(np_=1), dict(Sq=100)):
        assert _extp(**good, out=ODD) == ERR_ALIGN, good            # accepted by rules 1 - 4: seen as the next rule's code


def _i8(*s):
    return torch.zeros(s, dtype=torch.int8)


def test_extend_ops_and_modules_refuse_cpu_tensors_bad_strides_and_wide_groups():
    from autosmoothquant_amd import ops
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, Sq, Hq, Hkv, D, smax = 2, 3, 4, 2, 16, 8
    q, kc, vc = _i8(B, Sq, Hq, D), _i8(B, smax, Hkv, D), _i8(B, smax, Hkv, D)
    n, m = torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    att = Int8Attention(0.01, 0.02)
    for args, kw in (((q, kc, vc, n), {}), ((q, kc[:, :5], vc[:, :5], None), dict(q_len=m)), ((q, kc, vc, n), dict(q_len=m, max_len=3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.attn_extend_i8(*args[:4], 0.01, 0.02, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att.extend(q, kc, vc, n, m)
    bad = [
        dict(q=q.float()), dict(q=q[0]), dict(q=q[:, 0]), dict(q=_i8(B, Sq, Hq, 2 * D)[..., :D]), dict(q=_i8(B, 2 * Sq, Hq, D)[:, ::2]), dict(q=_i8(B + 1, Sq, Hq, D)),
        dict(q=_i8(B, Sq, 34, D)),                              # r = 17
        dict(q=_i8(B, Sq, 5, D)),                               # Hq no multiple of Hkv
        dict(q=_i8(B, Sq, Hq, 24), k_cache=_i8(B, smax, Hkv, 24), v_cache=_i8(B, smax, Hkv, 24)),      # D no multiple of 16
        dict(k_cache=kc.transpose(1, 2)), dict(k_cache=kc[:, ::2], v_cache=vc[:, ::2]), dict(k_cache=_i8(B, smax, Hkv, 2 * D)[..., :D]),
        dict(k_cache=kc[:, :5]),                                # the two caches disagree
        dict(v_cache=_i8(B, 2 * smax, Hkv, D)[:, :smax]),       # two batch pitches
        dict(v_cache=vc.to(torch.int16)),
        dict(kv_len=n.long()), dict(kv_len=torch.zeros(B + 1, dtype=torch.int32)), dict(kv_len=[1, 2]),
        dict(q_len=m.long()), dict(q_len=torch.zeros(B + 1, dtype=torch.int32)), dict(q_len=[1, 2]), dict(q_len=torch.zeros((B, 1), dtype=torch.int32)), dict(q_len=3),
        dict(max_len=smax + 1), dict(max_len=-1),
    ]
    for kw in bad:
        a = dict(q=q, k_cache=kc, v_cache=vc, kv_len=n, q_len=m, max_len=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_extend_i8(a["q"], a["k_cache"], a["v_cache"], a["kv_len"], 0.01, 0.02, q_len=a["q_len"], max_len=a["max_len"])
    with pytest.raises(ValueError):
        att.extend(q[:, 0], kc, vc, n)                          # the module takes [B, Sq, Hq, d]
    # the paged op: attn_decode_i8_paged's rules for the pools and the table
    NP, PS, TW = 6, 16, 3
    kp, vp, tab = _i8(NP, PS, Hkv, D), _i8(NP, PS, Hkv, D), torch.zeros((B, TW), dtype=torch.int32)
    wide = torch.zeros((B, TW + 2), dtype=torch.int32)
    for args, kw in (((q, kp, vp, tab, n), {}), ((q, kp, vp, wide[:, :TW], None), dict(q_len=m)), ((q, kp, vp, tab, n), dict(max_len=3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.attn_extend_i8_paged(*args, 0.01, 0.02, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att.extend_paged(q, kp, vp, tab, n, m)
    bad = [
        dict(q=q.float()), dict(q=q[0]), dict(q=_i8(B, Sq, Hq, 2 * D)[..., :D]), dict(q=_i8(B + 1, Sq, Hq, D)), dict(q=_i8(B, Sq, 34, D)), dict(q=_i8(B, Sq, 5, D)),
        dict(k_pool=kp.transpose(1, 2)), dict(k_pool=_i8(NP, 24, Hkv, D), v_pool=_i8(NP, 24, Hkv, D)), dict(k_pool=kp[:4]), dict(v_pool=_i8(NP, 2 * PS, Hkv, D)[:, :PS]),
        dict(block_table=tab.long()), dict(block_table=tab[0]), dict(block_table=torch.zeros((B + 1, TW), dtype=torch.int32)), dict(block_table=wide[:, ::2]),
        dict(kv_len=n.long()), dict(kv_len=[1, 2]), dict(q_len=m.long()), dict(q_len=torch.zeros(B + 1, dtype=torch.int32)), dict(q_len=[1, 2]),
        dict(max_len=TW * PS + 1), dict(max_len=-1),
    ]
    for kw in bad:
        a = dict(q=q, k_pool=kp, v_pool=vp, block_table=tab, kv_len=n, q_len=m, max_len=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.attn_extend_i8_paged(a["q"], a["k_pool"], a["v_pool"], a["block_table"], a["kv_len"], 0.01, 0.02, q_len=a["q_len"], max_len=a["max_len"])
    with pytest.raises(ValueError):
        att.extend_paged(q[0], kp, vp, tab, n)
    # decode keeps refusing Sq != 1; extend adds no state
    with pytest.raises(ValueError):
        att.decode(q, kc, vc, n)
    assert sorted(att.state_dict()) == ["pv_bmm.a", "qk_bmm.a"]


def test_ragged_cache_rewind():
    from autosmoothquant_amd.layers.nn.attention import RaggedInt8KVCache
    c = RaggedInt8KVCache(3, 8, 2, 16, device="cpu")
    ptr = c.kv_len.data_ptr()
    c.advance([7, 2, 3])
    c.k.fill_(7)
    c.rewind(2)
    assert c.kv_len.tolist() == c.lengths == [5, 0, 1] and c.bound() == 5
    c.rewind([3, 0, 1])
    assert c.kv_len.tolist() == c.lengths == [2, 0, 0]
    c.rewind(0)
    assert c.kv_len.tolist() == c.lengths == [2, 0, 0]
    for bad in (1, [3, 0, 0], [0, 0, 1], [1, 0], -1, [-1, 0, 0]):
        with pytest.raises(ValueError):
            c.rewind(bad)
        assert c.kv_len.tolist() == c.lengths == [2, 0, 0]      # a refused rewind moves nothing
    c.advance([4, 4, 4])
    assert c.kv_len.tolist() == c.lengths == [6, 4, 4]
    assert c.kv_len.data_ptr() == ptr and bool((c.k == 7).all())          # the device tensor stays where it is; rewind() forgets, it does not clear


def test_paged_cache_rewind():
    from autosmoothquant_amd.layers.nn.attention import PagedInt8KVCache
    NP, PS, Hkv, D, B, ML = 9, 16, 2, 16, 3, 70
    c = PagedInt8KVCache(NP, PS, Hkv, D, B, ML, device="cpu")
    ptrs = (c.block_table.data_ptr(), c.kv_len.data_ptr())
    state = lambda: (list(c.lengths), [list(p) for p in c.pages], list(c.free), c.kv_len.tolist(), c.block_table.tolist())  # noqa: E731
    c.reserve([30, 5, 16])
    c.advance([30, 5, 16])
    c.k.fill_(7)
    held = state()
    assert [len(p) for p in c.pages] == [2, 1, 1]
    c.reserve(4)                                                # a speculative step of 4 tokens: sequences 0 and 2 take a page each
    c.advance(4)
    assert [len(p) for p in c.pages] == [3, 1, 2] and c.lengths == [34, 9, 20]
    table = c.block_table.tolist()
    c.rewind(4)                                                 # all rejected: the free list is what it was before the step, newest page first
    assert state()[:4] == held[:4] and c.block_table.tolist() == table          # the stale entries stay behind the lengths
    c.reserve(4)
    c.advance(4)
    assert c.pages == [[0, 1, 4], [2], [3, 5]] and c.block_table.tolist() == table          # the same pages come back in the same order
    newest = (c.pages[0][-1], c.pages[2][-1])
    free = list(c.free)
    c.rewind([1, 0, 4])                                         # 33 keys keep sequence 0's third page; 16 keys give sequence 2's second page back
    assert c.lengths == c.kv_len.tolist() == [33, 9, 16] and [len(p) for p in c.pages] == [3, 1, 1] and c.free == free + [newest[1]]
    c.rewind([1, 9, 0])                                         # 32 keys: exactly two pages; an emptied sequence holds none
    assert c.lengths == [32, 0, 16] and [len(p) for p in c.pages] == [2, 0, 1] and c.free[-2:] == [held[1][1][0], newest[0]]
    before = state()
    for bad in (17, [33, 0, 0], [0, 1, 0], [1, 1], -1, [0, 0, -1]):
        with pytest.raises(ValueError):
            c.rewind(bad)
        assert state() == before                                # a refused call moves nothing
    held_pages = [p for pg in c.pages for p in pg]
    assert len(set(held_pages)) == len(held_pages) and sorted(held_pages + c.free) == list(range(NP))
    assert (c.block_table.data_ptr(), c.kv_len.data_ptr()) == ptrs and bool((c.k == 7).all())       # what a captured step reads stays where it is; nothing is cleared


def test_the_case_table_covers_what_it_promises():
    assert len(X.CASES) == 9 and len(X.PARAMS) == 9 * 3 * 2
    tiles = [X.tiling(c[1], c[2]) for c in X.CASES]
    assert {(c[3] + 63) // 64 for c in X.CASES} == {1, 2, 3, 4}
    assert {t[1] for t in tiles} == {4, 15, 16} and {t[0] for t in tiles} == {1, 2, 3, 4, 5, 8} and {t[2] for t in tiles} == {1, 2, 3}
    assert any(c[2] % t[0] for c, t in zip(X.CASES, tiles))    # a last token group that is partly filled
    assert [X.chunked(ci) for ci in range(9)] == [False, False, True, True, True, False, True, False, False]
    assert {X.chunk(ci) for ci in range(9) if X.chunked(ci)} == {1024, 1088}
    assert [R.chunk(16, 1 << 16), R.chunk(15, 1 << 16)] == [1024, 1088]
    assert any(m == 0 for c in X.CASES if c[5] for m in c[5])  # q_len of 0
    L9 = X.case_keys(8)
    assert X.CASES[8][4][0] == 3 and X.CASES[8][5][0] == 8 and L9[0].tolist() == [0, 0, 0, 0, 0, 1, 2, 3]       # m_b > n_b: the first five rows are zero
    for ci, (hkv, r, sq, d, lengths, q_len) in enumerate(X.CASES):
        L = X.case_keys(ci)
        assert L.shape == (len(lengths), sq) and 0 < int(L.max()) <= max(lengths) <= X.max_len(lengths)
        for b, n in enumerate(lengths):
            m = sq if q_len is None else q_len[b]
            assert L[b].tolist() == [max(n - m + s + 1, 0) if s < m else 0 for s in range(sq)]
    # row_keys clamps as the device does
    assert X.row_keys([50, -3, 7], [9, 2, -1], 4, 10).tolist() == [[7, 8, 9, 10], [0, 0, 0, 0], [0, 0, 0, 0]]
    # fold / unfold_rows are each other's inverse
    q = np.arange(2 * 7 * 6 * 16, dtype=np.int64).reshape(2, 7, 6, 16).astype(np.int8)
    for s in range(7):
        tg, rows = X.unfold_rows(3, 7, s)
        assert np.array_equal(X.fold(q, 3, tg)[:, rows(6)], q[:, s])
    assert not X.fold(q, 3, 1)[:, 6:15].any() and not X.fold(q, 3, 1)[:, 21:].any()          # tokens 7 .. 9 of the second group do not exist


@pytest.mark.parametrize("p", X.PARAMS, ids=[X.param_id(p) for p in X.PARAMS])
def test_the_yardstick_keeps_its_caps_on_every_gpu_case(p):
    case, si, sign = p
    s_lo, s_hi, nband, total = X.case_sums(case, si, sign)
    assert total == X.CASES[case][0] * X.CASES[case][1] * int(X.case_keys(case).sum())
    for pv in X.PV_ALPHAS:
        lo, hi = R.interval(s_lo, s_hi, pv)
        amb = R.caps(lo, hi, nband, total, f"{X.param_id(p)} pv_alpha {pv:.5f}")
        assert (lo <= hi).all()
        print(f"{X.param_id(p)} pv_alpha {pv:.5f}: band {nband} / {total}, ambiguous outputs {amb} / {lo.size}")


def test_the_reference_is_exact_on_the_staircases():
    for i, shape in enumerate(X.UNIFORM):
        q, k, v, lengths, q_len, ml, L, s = X.uniform_staircase(i)
        C = R.chunk(X.tiling(shape[1], shape[2])[1], ml)
        edges = set(L.reshape(-1).tolist())
        assert {16, 64, C} <= edges and {15, 17, 63, 65, C - 1, C + 1} & edges, shape          # a tile edge, a 64-key step, the chunk edge
        s_lo, s_hi, nband, total = X.expanded_sums(q, k, v, L, 0.01)
        assert nband == 0 and total > 0 and np.array_equal(s_lo, s_hi) and np.array_equal(s_lo, s), shape
        for b in range(L.shape[0]):                             # each token takes exactly one more V row than the one before it
            for t in range(1, L.shape[1]):
                if L[b, t] > 0 and L[b, t - 1] > 0 and np.rint(127.0 / L[b, t]) == np.rint(127.0 / L[b, t - 1]):
                    w = int(np.rint(127.0 / L[b, t]))
                    assert np.array_equal(s[b, t] - s[b, t - 1], w * v[b, L[b, t] - 1].astype(np.int64).repeat(shape[1], axis=0))
    for i, shape in enumerate(X.STAIRS):
        q, k, v, lengths, q_len, ml, L = X.poisoned_staircase(i)
        r = shape[1]
        assert (L > 0).any() and int(L.max()) == max(lengths)
        s_lo, s_hi, nband, total = X.expanded_sums(q, k, v, L, X.STAIR_ALPHA)
        assert nband == 0 and np.array_equal(s_lo, s_hi), shape
        for pv in X.EXACT_PVS:
            lo, hi = R.interval(s_lo, s_hi, pv)
            assert np.array_equal(lo, hi) and np.array_equal(lo, X.staircase_expected(v, L, r, pv)), shape
        for b in range(L.shape[0]):                             # the margin: a row's own last key leads every other key it sees by more than 20 / qk_alpha, and the
            for t in range(L.shape[1]):                         # key just behind its limit (the next token's, or the poison at n_b) would lead its own by as much
                if L[b, t] == 0:
                    continue
                for h in range(q.shape[2]):
                    sc = k[b, :L[b, t] + 1, h // r].astype(np.int64) @ q[b, t, h].astype(np.int64)
                    own, rest, nxt = sc[L[b, t] - 1], sc[:L[b, t] - 1], sc[L[b, t]]
                    assert (rest.size == 0 or (own - rest.max()) * X.STAIR_ALPHA > 20) and (nxt - own) * X.STAIR_ALPHA > 20, (shape, b, t, h)
    assert any((X.poisoned_staircase(i)[6] == 0).any() for i in range(len(X.STAIRS)))          # zero rows among them
