"""GPU: asq_rope_quantize_qkv_paged through ops.rope_quantize_qkv_paged (include/asq_hip_paged.h), and the paged decode step end to end.

  * every addressed pool row equals ops.rope_quantize_qkv_at writing the same tokens into a contiguous cache, for three dtypes, S = 1 and S = 37 with page edges
    inside the run (page sizes 16 and 48), under scattered tables; every other pool byte keeps guardband.pattern; q8 is bit-equal;
  * tokens out of range -- pos < 0, pos + s >= min(T, max_len), a page id of -1 or num_pages -- write nothing and zero their q8 rows, the tokens in range of the
    same call are unaffected;
  * end to end: a padded prefill and 20 decode steps through RopeQuantQKV + PagedInt8KVCache + Int8Attention.decode_paged, one sequence reset and re-admitted midway
    (freed pages are reused), every step bit-equal to the same run on RaggedInt8KVCache + Int8Attention.decode;
  * one captured step (append + decode) replayed three times while pos, kv_len and the table move in place, one replay crossing into a freshly reserved page."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import ops
from test_hip_rope_q8 import BF16, DEV, F16, F32, NAME, SCALES, _inputs, _tables

pytestmark = pytest.mark.gpu
# (B, S, Hq, Hkv, D), page size, positions: distinct per sequence; with S = 37 every run crosses at least one page edge (at 16: two or three)
SHAPES = [((1, 1, 1, 1, 16), 16, [0]), ((3, 1, 8, 2, 128), 16, [15, 16, 0]), ((4, 1, 4, 4, 64), 48, [47, 48, 95, 3]), ((3, 37, 4, 2, 64), 16, [0, 11, 16]),
          ((2, 37, 5, 1, 48), 48, [12, 47])]
CASES = [(dt, s, P, p) for dt in (F16, BF16, F32) for s, P, p in SHAPES]


def _pools(num_pages, P, Hkv, D, off):
    """two pools holding guardband.pattern (each at its own offset of the pattern) -> (pools, copies of what they hold)"""
    n = num_pages * P * Hkv * D
    pools = [GB.pattern(off + i * n, n, torch.device(DEV)).view(torch.int8).view(num_pages, P, Hkv, D).clone() for i in range(2)]
    return pools, [p.clone() for p in pools]


def _scattered_table(B, width, num_pages, seed):
    """[B, width] of distinct pages from a seeded permutation, the sequences' pages interleaved"""
    perm = torch.randperm(num_pages, generator=torch.Generator().manual_seed(seed)).tolist()
    t = torch.zeros((B, width), dtype=torch.int32)
    for j in range(width):
        for b in range(B):
            t[b, j] = perm.pop()
    return t


def _expect(want, host, cache, b, first, count, P):
    """rows first .. first + count - 1 of sequence b of the contiguous cache, copied to where the table puts them"""
    for c in range(first, first + count):
        want[int(host[b, c // P]), c % P] = cache[b, c]


@pytest.mark.parametrize("dt,shape,P,pos", CASES, ids=[f"{NAME[dt]}-" + "x".join(map(str, s)) + f"-page{P}" for dt, s, P, _ in CASES])
def test_equals_the_contiguous_append_row_by_row(dt, shape, P, pos):
    B, S, Hq, Hkv, D = shape
    q, k, v = _inputs(dt, shape, "fused")
    smax = max(pos) + S
    width = -(-smax // P)
    num_pages = B * width + 2
    cos, sin = _tables(smax + 2, D, dt)
    host = _scattered_table(B, width, num_pages, 53000 + S + P)
    tab, p = host.to(DEV), torch.tensor(pos, dtype=torch.int32, device=DEV)
    (kp, vp), (want_k, want_v) = _pools(num_pages, P, Hkv, D, 4096)
    kc, vc = (torch.zeros((B, smax, Hkv, D), dtype=torch.int8, device=DEV) for _ in range(2))
    q8_at, _, _ = ops.rope_quantize_qkv_at(q, k, v, cos, sin, *SCALES, p, kc, vc)
    q8, k_ret, v_ret = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, *SCALES, p, tab, kp, vp, max_len=smax)
    assert k_ret.data_ptr() == kp.data_ptr() and v_ret.data_ptr() == vp.data_ptr() and q8.dtype == torch.int8 and tuple(q8.shape) == (B, S, Hq, D) and q8.is_contiguous()
    assert torch.equal(q8, q8_at), "q8 differs from the contiguous append"
    for b in range(B):
        _expect(want_k, host, kc, b, pos[b], S, P), _expect(want_v, host, vc, b, pos[b], S, P)
    assert torch.equal(kp, want_k) and torch.equal(vp, want_v), "a pool differs from its pattern with each token's row written"
    assert int(q8.max()) == 127 and int(q8.min()) == -128       # planted +-inf / +-max-finite saturate


@pytest.mark.parametrize("dt", [F16, F32], ids=["f16", "f32"])
def test_out_of_range_tokens_write_nothing(dt):
    B, S, Hq, Hkv, D, P, width = 8, 4, 4, 2, 32, 16, 2
    num_pages = B * width
    q, k, v = _inputs(dt, (B, S, Hq, Hkv, D), "dense")
    for T, ml in ((30, 27), (25, 32)):                          # max_len, then the tables, are the shorter bound
        lim = min(T, ml)
        cos, sin = _tables(T, D, dt)
        pos = [-1, lim - 2, lim, 1 << 30, -(1 << 31), 3, 14, 13]   # out, two tokens in, out, out, out, in, in with a bad second page, in with a bad first page
        host = _scattered_table(B, width, num_pages, 53100 + T)
        host[6, 1], host[7, 0] = -1, num_pages
        p = torch.tensor(pos, dtype=torch.int32, device=DEV)
        (kp, vp), (want_k, want_v) = _pools(num_pages, P, Hkv, D, 8192)
        kc, vc = (torch.zeros((B, 40, Hkv, D), dtype=torch.int8, device=DEV) for _ in range(2))
        q8, _, _ = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, *SCALES, p, host.to(DEV), kp, vp, max_len=ml)
        want_q = torch.zeros_like(q8)
        for b, s0, t in ((1, 0, 2), (5, 0, S), (6, 0, 2), (7, 3, 1)):      # (sequence, first token in range, tokens in range)
            w = ops.rope_quantize_qkv(q[b:b + 1, s0:s0 + t], k[b:b + 1, s0:s0 + t], v[b:b + 1, s0:s0 + t], cos, sin, *SCALES, pos=pos[b] + s0)
            want_q[b, s0:s0 + t] = w[0][0]
            kc[b, pos[b] + s0:pos[b] + s0 + t], vc[b, pos[b] + s0:pos[b] + s0 + t] = w[1][0], w[2][0]
            _expect(want_k, host, kc, b, pos[b] + s0, t, P), _expect(want_v, host, vc, b, pos[b] + s0, t, P)
        assert torch.equal(q8, want_q), f"T = {T}, max_len = {ml}: q8 rows of skipped tokens are not zero, or those in range differ"
        assert torch.equal(kp, want_k) and torch.equal(vp, want_v), f"T = {T}, max_len = {ml}: a token out of range wrote into a pool"


def _step_inputs(g, B, S, Hq, Hkv, D, dt):
    fused = (torch.randn((B, S, (Hq + 2 * Hkv) * D), generator=g) * 2).to(dt).to(DEV)
    return [fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv))]


def test_paged_prefill_and_decode_end_to_end_equals_the_ragged_cache():
    """B = 3, prompts of 5 / 21 / 12 tokens as one padded prefill, ten single-token steps, sequence 1 reset and re-admitted with a 7-token prompt, ten more steps; 4 / 2
    heads of d = 64, pages of 16 in a pool of 12.  After every call q8 and each sequence's gathered rows equal the RaggedInt8KVCache run's, and every decode step's
    output is bit-equal to Int8Attention.decode on the ragged cache with the same max_len."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, PagedInt8KVCache, RaggedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, P, ml, prompts, dt = 3, 4, 2, 64, 16, 80, [5, 21, 12], F16
    qs, ks, vs = 0.037, 0.011, 0.073
    g = torch.Generator().manual_seed(53200)
    cos, sin = _tables(ml, D, dt)
    mod = RopeQuantQKV(qs, ks, vs).to(DEV)
    att = Int8Attention.from_scale(qs, ks, vs, 0.05, sm_scale=D ** -0.5, causal=True).to(DEV)
    ragged = RaggedInt8KVCache(B, ml, Hkv, D, device=DEV)
    paged = PagedInt8KVCache(12, P, Hkv, D, B, ml, device=DEV)
    ptrs = (paged.block_table.data_ptr(), paged.kv_len.data_ptr())
    plan = [(max(prompts), prompts)] + [(1, None)] * 10 + [("reset", 1), (7, [0, 7, 0])] + [(1, None)] * 10
    freed, steps = None, 0
    for S, adv in plan:
        if S == "reset":
            freed = list(paged.pages[adv])
            ragged.reset(adv), paged.reset(adv)
            continue
        q, k, v = _step_inputs(g, B, S, Hq, Hkv, D, dt)
        q8r, _, _ = mod(q, k, v, cos, sin, cache=ragged, advance=adv)
        q8p, kp, vp = mod(q, k, v, cos, sin, cache=paged, advance=adv)
        assert kp.data_ptr() == paged.k.data_ptr() and vp.data_ptr() == paged.v.data_ptr()
        assert torch.equal(q8p, q8r) and paged.lengths == ragged.lengths and paged.kv_len.tolist() == paged.lengths
        for b in range(B):
            gk, gv = paged.gather(b)
            n = ragged.lengths[b]
            assert torch.equal(gk, ragged.k[b, :n]) and torch.equal(gv, ragged.v[b, :n]), f"sequence {b}: the gathered pages differ from the ragged cache's rows"
        if adv == [0, 7, 0]:
            assert paged.pages[1][0] in freed                   # the re-admitted sequence got a page it had given back
        if S == 1:
            steps += 1
            want = att.decode(q8r, ragged.k, ragged.v, ragged.kv_len, max_len=ragged.bound())
            got = att.decode_paged(q8p, paged.k, paged.v, paged.block_table, paged.kv_len, max_len=paged.bound())
            assert tuple(got.shape) == (B, 1, Hq, D) and torch.equal(got, want), f"decode step {steps}: the paged output differs from the ragged cache's"
            assert int(got.abs().max()) > 10                    # the scales leave a signal
    assert steps == 20 and set(freed) <= set(paged.pages[1]) and (paged.block_table.data_ptr(), paged.kv_len.data_ptr()) == ptrs
    held = [p for pg in paged.pages for p in pg]
    assert len(set(held)) == len(held)


def test_a_captured_paged_step_replays_as_positions_lengths_and_the_table_move():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, PagedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, P, ml, start = 3, 4, 2, 64, 16, 64, [15, 3, 30]
    g = torch.Generator().manual_seed(53300)
    cos, sin = _tables(ml, D, F16)
    mod = RopeQuantQKV(*SCALES).to(DEV)
    att = Int8Attention(0.001, 1.0 / 127).to(DEV)
    pre = _step_inputs(g, B, max(start), Hq, Hkv, D, F16)
    q, k, v = _step_inputs(g, B, 1, Hq, Hkv, D, F16)
    caches = [PagedInt8KVCache(10, P, Hkv, D, B, ml, device=DEV) for _ in range(2)]
    for c in caches:
        mod(*pre, cos, sin, cache=c, advance=start)
    cap, eager = caches

    def step(c, n):
        q8, _, _ = ops.rope_quantize_qkv_paged(q, k, v, cos, sin, *SCALES, c.kv_len, c.block_table, c.k, c.v, max_len=ml)
        return att.decode_paged(q8, c.k, c.v, c.block_table, n, max_len=ml)

    n_cap, n_eager = cap.kv_len + 1, eager.kv_len + 1
    warm = PagedInt8KVCache(10, P, Hkv, D, B, ml, device=DEV)
    warm.reserve(1)
    step(warm, warm.kv_len + 1)                                 # (the first call sets the kernel's LDS attribute: not inside a capture)
    torch.cuda.synchronize()
    cap.reserve(1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # append + decode on one stream: no parallel branches
        out = step(cap, n_cap)
    outs, fresh = [], []
    for it in range(3):
        before = [len(pg) for pg in cap.pages]
        cap.reserve(1)                                          # writes the table in place (nothing to do for the first replay: reserved above)
        fresh.append([len(pg) - m for pg, m in zip(cap.pages, before)])
        graph.replay()
        outs.append(out.clone())
        cap.advance(1), n_cap.add_(1)
    torch.cuda.synchronize()
    assert fresh == [[0, 0, 0], [0, 0, 0], [0, 0, 1]]           # the third replay wrote position 32 of sequence 2: the first row of a page reserved after the capture
    for it in range(3):                                         # the same three steps, eagerly
        eager.reserve(1)
        assert torch.equal(step(eager, n_eager), outs[it]), f"replay {it} differs from the eager step"
        eager.advance(1), n_eager.add_(1)
    assert cap.lengths == eager.lengths == [18, 6, 33] and cap.kv_len.tolist() == cap.lengths
    for b in range(B):
        for x, y in zip(cap.gather(b), eager.gather(b)):
            assert torch.equal(x, y)
