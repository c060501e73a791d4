"""GPU: the pitched entries at byte offsets beyond 2^31 and 2^32 (tests/far_offsets.py states the rule: whole equals parts, bit for bit, on the device).

Little data is touched; the span comes from a pitch.

  * the ragged cache: three sequences at a kv_batch_pitch just under 2^31 (a multiple of 16, no multiple of Hkv * D), so that sequence 1's rows straddle byte 2^31 and
    sequence 2's byte 2^32 -- ops.attn_decode_i8, ops.attn_extend_i8 (Sq = 3, one padded sequence), ops.rope_quantize_qkv into k_out / v_out slot views and
    ops.rope_quantize_qkv_at, each against the same call on a dense [3, Smax, Hkv, D] cache holding the same bytes; Hq / Hkv = 4 / 2 with D = 64, r = 1 with D = 128,
    and decode at r = 7 just over its chunk of 2304 keys;
  * paged pools of just over 2^32 / pitch pages (page size 16; the dense pitch, and a padded one that is no power of two): the tables name page 0, the pages on each
    side of 2^31 and of 2^32, the last page and a partial one -- ops.attn_decode_i8_paged, ops.attn_extend_i8_paged and ops.rope_quantize_qkv_paged against the same
    calls on compact pools with the ids remapped to 0 .. n - 1; decode at r = 7 over 2310 keys;
  * a block table whose row stride puts row 1 beyond byte 2^31 and row 2 beyond 2^32;
  * ops.rope and ops.rope_quantize_qkv on [1, 3, H, D] views with a row pitch of 2^31 + 64 bytes, fp16 and fp32, q, k and v in turn, against dense copies.

Every far tensor sits 2^31 bytes into an arena of 0x55 (far_offsets.Arena); after the calls the apron, the pitch gaps and every pool byte outside the named pages are
what they were.  The CPU anchors: attn_decode_ref.sums / attn_extend_ref.expanded_sums intervals for the attention outputs (the caches here are a few hundred keys:
all of them go through), and for the appends the two launches they replace (ops.rope then ops.quantize_act on dense tokens: test_hip_rope_q8._composition)."""
import pytest
import torch

import attn_decode_ref as R
import attn_extend_ref as E
import far_offsets as F
from autosmoothquant_amd import ops
from test_hip_rope_q8 import DEV, F16, F32, NAME, SCALES, _composition, _inputs, _tables

pytestmark = pytest.mark.gpu
SHAPES = {"small": F.KV_SMALL, "r1": F.KV_R1, "chunked": F.KV_CHUNKED}
PV = R.PV_ALPHAS[0]
P = F.PAGE


def _alpha(d):
    return R.SR.alphas((1, 1, d))[1]


def _q(shape, seed):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _i32(values):
    return torch.tensor(list(values), dtype=torch.int32, device=DEV)


def _check_decode(got, q, k, v, lengths, alpha, what):
    """the CPU anchor: got inside attn_decode_ref's interval for these operands (k, v: contiguous caches)"""
    s_lo, s_hi, _, _ = R.sums(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), tuple(lengths), alpha)
    R.check(got.cpu().numpy(), *R.interval(s_lo, s_hi, PV), what)
    assert int(got.abs().max()) > 0


def _check_extend(got, q, k, v, lengths, q_len, alpha, what):
    L = E.row_keys(lengths, q_len, q.shape[1], k.shape[1])
    s_lo, s_hi, _, _ = E.expanded_sums(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), L, alpha)
    R.check(got.cpu().numpy(), *R.interval(s_lo, s_hi, PV), what)
    assert int(got.abs().max()) > 0


# ---- the ragged cache ----------------------------------------------------------------------------------------------------------------------------------------------

class Ragged:
    """k and v caches [3, smax, Hkv, D] at far_offsets.ragged_pitch, each in its own arena, the rows random, the gaps 0x55; .dense: contiguous copies"""

    def __init__(self, s, seed):
        self.Hq, self.Hkv, self.D, self.smax, self.lengths = s["Hq"], s["Hkv"], s["D"], s["smax"], s["lengths"]
        self.row = self.Hkv * self.D
        self.bytes = self.smax * self.row
        self.pitch = F.ragged_pitch(self.smax, self.row)
        self.arenas = [F.Arena(2 * self.pitch + self.bytes, DEV) for _ in range(2)]
        for i, ar in enumerate(self.arenas):
            for b in range(3):
                ar.fill_random(b * self.pitch, b * self.pitch + self.bytes, seed + 10 * i + b)
        self.far = [ar.view(torch.int8, (3, self.smax, self.Hkv, self.D), (self.pitch, self.row, self.D, 1)) for ar in self.arenas]
        self.dense = [c.contiguous() for c in self.far]
        assert all(c.stride(0) == self.pitch and c.stride(0) % 16 == 0 and c.stride(0) % self.row for c in self.far) and all(c.is_contiguous() for c in self.dense)
        self.edge_rows = [0, (F.G31 - self.pitch) // self.row, 2 * (F.G31 - self.pitch) // self.row]     # sequence b's row that holds byte b * 2^31
        for b in (1, 2):
            assert b * self.pitch < b * F.G31 < b * self.pitch + self.bytes and 2 <= self.edge_rows[b] < self.lengths[b] - 2
            for ar in self.arenas:
                for r in range(self.edge_rows[b] - 1, self.edge_rows[b] + 2):
                    ar.differs_below(b * self.pitch + r * self.row, self.row)

    def intact(self):
        """the aprons and both pitch gaps still hold 0x55"""
        return all(ar.apron_intact() and ar.is_fill(self.bytes, self.pitch) and ar.is_fill(self.pitch + self.bytes, 2 * self.pitch) for ar in self.arenas)

    def equal(self):
        return all(torch.equal(f, d) for f, d in zip(self.far, self.dense))


@pytest.mark.parametrize("tag", list(SHAPES))
def test_ragged_decode_equals_the_dense_cache(tag):
    """peak: two arenas of 2^31 + 2 * pitch bytes, 12.1 GiB; k_cache and v_cache cross 2^31 (sequence 1) and 2^32 (sequence 2)"""
    F.need(F.case(f"ragged-{tag}").peak, f"ragged decode, {tag}")
    c = Ragged(SHAPES[tag], 61000)
    if tag == "chunked":
        assert max(c.lengths) > R.chunk(c.Hq // c.Hkv, c.smax) == 2304
    q, kv_len, alpha = _q((3, c.Hq, c.D), 61001), _i32(c.lengths), _alpha(c.D)
    got = ops.attn_decode_i8(q, *c.far, kv_len, alpha, PV)
    want = ops.attn_decode_i8(q, *c.dense, kv_len, alpha, PV)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} output bytes differ between the far-pitched and the dense cache"
    _check_decode(got, q, *c.dense, c.lengths, alpha, f"ragged decode, {tag}")
    assert c.equal() and c.intact()
    del c, got, want
    F.release()


@pytest.mark.parametrize("tag", ["small", "r1"])
def test_ragged_extend_equals_the_dense_cache(tag):
    """peak 12.1 GiB; k_cache and v_cache cross 2^31 and 2^32"""
    F.need(F.case(f"ragged-{tag}").peak, f"ragged extend, {tag}")
    c = Ragged(SHAPES[tag], 61100)
    q_len = [3, 2, 3]                                           # sequence 1 is padded: its last token counts for nothing
    q, kv_len, ql, alpha = _q((3, 3, c.Hq, c.D), 61101), _i32(c.lengths), _i32(q_len), _alpha(c.D)
    got = ops.attn_extend_i8(q, *c.far, kv_len, alpha, PV, q_len=ql)
    want = ops.attn_extend_i8(q, *c.dense, kv_len, alpha, PV, q_len=ql)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} output bytes differ between the far-pitched and the dense cache"
    assert not got[1, 2].any()
    _check_extend(got, q, *c.dense, c.lengths, q_len, alpha, f"ragged extend, {tag}")
    assert c.equal() and c.intact()
    del c, got, want
    F.release()


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("tag", ["small", "r1"])
def test_ragged_appends_equal_the_dense_cache(tag, dt):
    """peak 12.1 GiB; the written k_cache / v_cache rows straddle 2^31 (sequence 1) and 2^32 (sequence 2).  rope_quantize_qkv writes one slot for all sequences: it
    runs twice, on each edge; rope_quantize_qkv_at takes both edges and the cache's last rows in one call"""
    F.need(F.case(f"ragged-{tag}").peak, f"ragged appends, {tag}")
    c = Ragged(SHAPES[tag], 61200)
    S = 5
    q, k, v = _inputs(dt, (3, S, c.Hq, c.Hkv, c.D), "dense")
    cos, sin = _tables(c.smax, c.D, dt)
    for pos in (c.edge_rows[1] - 2, c.edge_rows[2] - 2):
        got = ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos, k_out=c.far[0][:, pos:pos + S], v_out=c.far[1][:, pos:pos + S])
        want = ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos, k_out=c.dense[0][:, pos:pos + S], v_out=c.dense[1][:, pos:pos + S])
        assert got[1].data_ptr() == c.far[0][:, pos:pos + S].data_ptr() and torch.equal(got[0], want[0]) and c.equal(), f"rope_quantize_qkv at pos {pos}"
        for name, g, w in zip("qkv", (got[0], c.far[0][:, pos:pos + S], c.far[1][:, pos:pos + S]), _composition(q, k, v, cos, sin, pos)):
            assert torch.equal(g, w), f"{name}8 at pos {pos} differs from rope + quantize_act"
        assert c.intact(), f"rope_quantize_qkv at pos {pos} wrote outside its slots"
    q, k, v = _inputs(dt, (3, S, c.Hq, c.Hkv, c.D), "fused")
    pos = [c.smax - S, c.edge_rows[1] - 2, c.edge_rows[2] - 2]
    got = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, _i32(pos), *c.far)
    want = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, _i32(pos), *c.dense)
    assert torch.equal(got[0], want[0]) and c.equal(), "rope_quantize_qkv_at"
    for b in range(3):
        w = _composition(q[b:b + 1], k[b:b + 1], v[b:b + 1], cos, sin, pos[b])
        for name, g, ww in zip("qkv", (got[0][b:b + 1], c.far[0][b:b + 1, pos[b]:pos[b] + S], c.far[1][b:b + 1, pos[b]:pos[b] + S]), w):
            assert torch.equal(g, ww), f"rope_quantize_qkv_at: {name}8 of sequence {b} differs from rope + quantize_act"
    assert c.intact(), "rope_quantize_qkv_at wrote outside its rows"
    del c, got, want
    F.release()


# ---- paged pools ---------------------------------------------------------------------------------------------------------------------------------------------------

class Pools:
    """k and v pools [num_pages, 16, Hkv, D] of just over 2^32 bytes, each in its own arena, random throughout (a padded pitch's gaps too)"""

    def __init__(self, hkv, d, pad, seed):
        self.hkv, self.d, self.seed = hkv, d, seed
        self.page = hkv * d * P
        self.pitch = self.page + pad
        self.n = F.pool_pages(self.pitch)
        self.arenas = [F.Arena(self.n * self.pitch, DEV) for _ in range(2)]
        for i, ar in enumerate(self.arenas):
            ar.fill_random(0, self.n * self.pitch, seed + i)
        self.far = [ar.view(torch.int8, (self.n, P, hkv, d), (self.pitch, hkv * d, d, 1)) for ar in self.arenas]
        self.special = F.special_pages(self.pitch, self.n)

    def compact(self, ids):
        """dense pools holding the named pages in the order given, and far id -> compact id"""
        assert len(set(ids)) == len(ids) and min(ids) >= 0 and max(ids) < self.n
        idx = torch.tensor(ids, dtype=torch.int64, device=DEV)
        for i in ids:
            if i * self.pitch >= F.G31:
                for ar in self.arenas:
                    ar.differs_below(i * self.pitch, 256)
        return [p[idx].contiguous() for p in self.far], {i: j for j, i in enumerate(ids)}

    def pages_equal(self, ids, compact):
        idx = torch.tensor(ids, dtype=torch.int64, device=DEV)
        return all(torch.equal(p[idx], c) for p, c in zip(self.far, compact))

    def rest_intact(self, ids):
        """the aprons are 0x55 and every pool byte outside the named pages (the pitch gaps behind them too) is what fill_random wrote"""
        skip = [(i * self.pitch, i * self.pitch + self.page) for i in ids]
        return all(ar.apron_intact() and ar.is_random(0, self.n * self.pitch, self.seed + i, skip) for i, ar in enumerate(self.arenas))


def _tables_for(pool, rows):
    """[B, T] far ids: rows[b] is a list of page ids; a [:, :T] view of a wider table whose spare columns hold ids that must not be read; and the compact twin"""
    ids = [i for row in rows for i in row]
    compact, remap = pool.compact(ids)
    T = len(rows[0])
    wide = torch.full((len(rows), T + 5), pool.n - 2, dtype=torch.int32)
    wide_c = torch.full((len(rows), T + 5), len(ids) - 1, dtype=torch.int32)
    for b, row in enumerate(rows):
        wide[b, :T] = torch.tensor(row, dtype=torch.int32)
        wide_c[b, :T] = torch.tensor([remap[i] for i in row], dtype=torch.int32)
    return ids, compact, wide.to(DEV)[:, :T], wide_c.to(DEV)[:, :T]


def _gather(compact, tab_c, ml):
    """contiguous [B, ml, Hkv, D] caches holding each sequence's pages end to end"""
    return [c[tab_c.long()].flatten(1, 2)[:, :ml].contiguous() for c in compact]


def _small_rows(pool):
    """sequence 0: the special pages and page 1 (partial); sequence 1: their neighbours seven pages off, in reverse, and page 3"""
    other = [i + 7 if i + 7 < pool.n else i - 7 for i in pool.special][::-1]
    rows = [pool.special + [1], other + [3]]
    assert len({i for r in rows for i in r}) == 2 * len(rows[0])
    return rows


@pytest.mark.parametrize("pad", [0, F.POOL_PAD], ids=["dense", "padded"])
def test_paged_attention_equals_the_compact_pool(pad):
    """peak: two arenas of 2^31 + 2^32 bytes, 12.1 GiB, + 0.5 GiB of compare buffers; k_pool and v_pool cross 2^31 and 2^32"""
    F.need(F.case("paged-padded" if pad else "paged-dense").peak, "paged attention")
    Hq, Hkv, D = 4, 2, 64
    pool = Pools(Hkv, D, pad, 62000)
    assert pool.pitch & (pool.pitch - 1) or not pad
    rows = _small_rows(pool)
    T = len(rows[0])
    ids, compact, tab, tab_c = _tables_for(pool, rows)
    ml, lengths, alpha = T * P, [(T - 1) * P + 5, T * P], _alpha(D)
    kv_len = _i32(lengths)
    q = _q((2, Hq, D), 62001)
    got = ops.attn_decode_i8_paged(q, *pool.far, tab, kv_len, alpha, PV, max_len=ml)
    want = ops.attn_decode_i8_paged(q, *compact, tab_c, kv_len, alpha, PV, max_len=ml)
    assert torch.equal(got, want), f"decode: {int((got != want).sum())} of {got.numel()} output bytes differ between the far pool and the compact one"
    caches = _gather(compact, tab_c, ml)
    _check_decode(got, q, *caches, lengths, alpha, "paged decode")
    q3, q_len = _q((2, 3, Hq, D), 62002), [3, 2]
    got = ops.attn_extend_i8_paged(q3, *pool.far, tab, kv_len, alpha, PV, q_len=_i32(q_len), max_len=ml)
    want = ops.attn_extend_i8_paged(q3, *compact, tab_c, kv_len, alpha, PV, q_len=_i32(q_len), max_len=ml)
    assert torch.equal(got, want), f"extend: {int((got != want).sum())} of {got.numel()} output bytes differ between the far pool and the compact one"
    _check_extend(got, q3, *caches, lengths, q_len, alpha, "paged extend")
    assert pool.pages_equal(ids, compact) and pool.rest_intact(())
    del pool, compact, caches, got, want
    F.release()


def test_paged_chunked_decode_equals_the_compact_pool():
    """r = 7, D = 128, 2310 keys in 145 pages (the special ones among them), just over the chunk of 2304; peak 12.6 GiB; k_pool and v_pool cross 2^31 and 2^32"""
    F.need(F.case("paged-chunked").peak, "paged chunked decode")
    Hq, Hkv, D, n = 7, 1, 128, 2310
    pool = Pools(Hkv, D, 0, 62100)
    T = -(-(n + 3) // P)
    assert n > R.chunk(7, T * P) == 2304
    spread = [i for i in torch.randperm(pool.n, generator=torch.Generator().manual_seed(62101)).tolist()[:2 * T + 8] if i not in pool.special]
    mixed = pool.special + spread[:T - len(pool.special)]
    order = torch.randperm(T, generator=torch.Generator().manual_seed(62102)).tolist()
    rows = [[mixed[i] for i in order], spread[T:2 * T]]
    ids, compact, tab, tab_c = _tables_for(pool, rows)
    ml, lengths, alpha = T * P, [n, 17], _alpha(D)
    q = _q((2, Hq, D), 62103)
    got = ops.attn_decode_i8_paged(q, *pool.far, tab, _i32(lengths), alpha, PV, max_len=ml)
    want = ops.attn_decode_i8_paged(q, *compact, tab_c, _i32(lengths), alpha, PV, max_len=ml)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} output bytes differ between the far pool and the compact one"
    _check_decode(got, q, *_gather(compact, tab_c, ml), lengths, alpha, "paged chunked decode")
    assert pool.pages_equal(ids, compact) and pool.rest_intact(())
    del pool, compact, got, want
    F.release()


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
@pytest.mark.parametrize("pad", [0, F.POOL_PAD], ids=["dense", "padded"])
def test_paged_append_equals_the_compact_pool(pad, dt):
    """a prefill of T * 16 - 3 tokens per sequence from positions 0 and 3: every named page is written, the last of sequence 0 in part.  Peak 12.6 GiB; the written
    k_pool / v_pool pages lie on each side of 2^31 and 2^32"""
    F.need(F.case("paged-padded" if pad else "paged-dense").peak, "paged append")
    Hq, Hkv, D = 4, 2, 64
    pool = Pools(Hkv, D, pad, 62200)
    rows = _small_rows(pool)
    T = len(rows[0])
    ids, compact, tab, tab_c = _tables_for(pool, rows)
    ml, S, pos = T * P, T * P - 3, [0, 3]
    q, k, v = _inputs(dt, (2, S, Hq, Hkv, D), "fused")
    cos, sin = _tables(ml, D, dt)
    got = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, *SCALES, _i32(pos), tab, *pool.far, max_len=ml)
    want = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, *SCALES, _i32(pos), tab_c, *compact, max_len=ml)
    assert torch.equal(got[0], want[0]), "q8 differs between the far pool and the compact one"
    assert pool.pages_equal(ids, compact), "a written page differs between the far pool and the compact one"
    assert pool.rest_intact(ids), "the append wrote outside the named pages"
    caches = _gather(compact, tab_c, ml)
    for b in range(2):
        w = _composition(q[b:b + 1], k[b:b + 1], v[b:b + 1], cos, sin, pos[b])
        for name, g, ww in zip("qkv", (got[0][b:b + 1], caches[0][b:b + 1, pos[b]:pos[b] + S], caches[1][b:b + 1, pos[b]:pos[b] + S]), w):
            assert torch.equal(g, ww), f"{name}8 of sequence {b} differs from rope + quantize_act"
    del pool, compact, caches, got, want
    F.release()


def test_a_block_table_whose_rows_lie_beyond_2g_and_4g():
    """B = 3 with a table row stride of 2^29 + 8 entries: row 1 starts at byte 2^31 + 32, row 2 at 2^32 + 64.  The table sits behind an apron (a sign-extended row
    offset reads 0x55555555, an id that clamps to the last page) and holds random ids throughout (an unsigned wrap reads other pages).  Peak 8.3 GiB; block_table
    crosses 2^31 and 2^32; the pools are small"""
    F.need(F.case("paged-wide-table").peak, "wide block table")
    Hq, Hkv, D, T, num_pages = 4, 2, 64, 7, 64
    ar = F.Arena(3 * F.TABLE_PITCH * 4, DEV)
    whole = ar.view(torch.int32, (3 * F.TABLE_PITCH,))
    whole.random_(0, num_pages, generator=torch.Generator(device=DEV).manual_seed(62300))
    tab = ar.view(torch.int32, (3, T), (F.TABLE_PITCH, 1))
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(62301))[:3 * T].to(torch.int32).view(3, T)
    tab.copy_(perm.to(DEV))
    for b in (1, 2):
        ar.differs_below(b * F.TABLE_PITCH * 4, T * 4)
    dense_tab = tab.contiguous()
    assert tab.stride(0) == F.TABLE_PITCH and dense_tab.stride(0) == T
    pools = [_q((num_pages, P, Hkv, D), 62302 + i) for i in range(2)]
    ml, lengths, alpha = T * P, [T * P, 50, T * P - 11], _alpha(D)
    kv_len = _i32(lengths)
    q = _q((3, Hq, D), 62304)
    got = ops.attn_decode_i8_paged(q, *pools, tab, kv_len, alpha, PV, max_len=ml)
    assert torch.equal(got, ops.attn_decode_i8_paged(q, *pools, dense_tab, kv_len, alpha, PV, max_len=ml)), "decode"
    _check_decode(got, q, *_gather(pools, dense_tab, ml), lengths, alpha, "decode through the wide table")
    q3 = _q((3, 3, Hq, D), 62305)
    got = ops.attn_extend_i8_paged(q3, *pools, tab, kv_len, alpha, PV, max_len=ml)
    assert torch.equal(got, ops.attn_extend_i8_paged(q3, *pools, dense_tab, kv_len, alpha, PV, max_len=ml)), "extend"
    S, pos = 37, [ml - 37, 3, 40]
    x = _inputs(F16, (3, S, Hq, Hkv, D), "dense")
    cos, sin = _tables(ml, D, F16)
    far_pools, dense_pools = [p.clone() for p in pools], [p.clone() for p in pools]
    got = ops.rope_quantize_qkv_paged(*x, cos, sin, *SCALES, _i32(pos), tab, *far_pools, max_len=ml)
    want = ops.rope_quantize_qkv_paged(*x, cos, sin, *SCALES, _i32(pos), dense_tab, *dense_pools, max_len=ml)
    assert torch.equal(got[0], want[0]) and all(torch.equal(a, b) for a, b in zip(far_pools, dense_pools)), "append"
    assert not torch.equal(far_pools[0], pools[0])
    assert ar.apron_intact() and torch.equal(tab, dense_tab)
    del ar, whole, tab, pools, far_pools, dense_pools, got, want
    F.release()


# ---- input pitches -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_rope_inputs_at_a_row_pitch_beyond_2g(dt):
    """[1, 3, H, D] views whose rows lie 2^31 + 64 bytes apart: row 1 in [2^31, 2^32), row 2 beyond 2^32.  q, k and v take the pitch in turn (one arena), the other two
    stay dense; ops.rope on the same view.  Peak 6.1 GiB; the far input crosses 2^31 and 2^32, every output is small"""
    F.need(F.case(f"input-pitch-{NAME[dt]}").peak, "rope input pitch")
    Hq, Hkv, D, S, pos = 4, 2, 64, 3, 2
    es = torch.empty((), dtype=dt).element_size()
    ld = F.IN_PITCH // es
    dense = _inputs(dt, (1, S, Hq, Hkv, D), "dense")
    cos, sin = _tables(pos + S + 1, D, dt)
    want = ops.rope_quantize_qkv(*dense, cos, sin, *SCALES, pos=pos)
    for name, w, c in zip("qkv", want, _composition(*dense, cos, sin, pos)):
        assert torch.equal(w, c), f"{name}8 of the dense call differs from rope + quantize_act"
    ar = F.Arena(2 * F.IN_PITCH + Hq * D * es, DEV)
    for i, name in enumerate("qkv"):
        H = dense[i].shape[2]
        x = ar.view(dt, (1, S, H, D), (S * ld, ld, D, 1))
        x.copy_(dense[i])
        assert x.stride(1) * es == F.IN_PITCH and not x.is_contiguous()
        for r in (1, 2):
            ar.differs_below(r * F.IN_PITCH, H * D * es)
        ops_in = list(dense)
        ops_in[i] = x
        got = ops.rope_quantize_qkv(*ops_in, cos, sin, *SCALES, pos=pos)
        for n2, g, w in zip("qkv", got, want):
            assert torch.equal(g, w), f"{name} at the far pitch: {n2}8 differs from the dense call"
        c3, s3 = cos[:S].contiguous(), sin[:S].contiguous()
        bits = torch.int16 if es == 2 else torch.int32           # (the inputs hold NaN: bit patterns are compared)
        assert torch.equal(ops.rope(x, c3, s3).view(bits), ops.rope(dense[i], c3, s3).view(bits)), f"ops.rope of {name} at the far pitch differs from the dense call"
        assert torch.equal(x.view(bits), dense[i].view(bits))
        x.view(bits).fill_(int.from_bytes(bytes([F.FILL]) * es, "little"))
        assert ar.is_fill(-F.APRON, ar.span), f"{name} at the far pitch: a byte outside the three rows was written"
    del ar, x, got, want
    F.release()
