"""GPU: asq_attn_extend_i8 through ops.attn_extend_i8 / Int8Attention.extend (include/asq_hip_extend.h; the paged entry: tests/test_hip_attn_extend_paged.py).

  * the byte-level identities the kernel's structure gives: (I1) Sq = 1 is asq_attn_decode_i8; (I2) any Sq, one-pass and chunked, is the single-token
    entry given the same tile rows as "heads", token by token with kv_len' = L; (I3) where nothing is chunked, token s is attn_decode_i8(q[:, s], kv_len = L);
  * every case of tests/attn_extend_ref.py by the interval rule over the row-expanded problem, within its caps, under both signs of qk_alpha;
  * the two staircases, exact: uniform (q = 0: each token takes exactly one more V row) and poisoned (each token one-hot on its OWN last key: a key limit off by one
    either way, or a read behind n_b, moves every byte), with L on a tile edge, a 64-key step and the R-row chunk edge;
  * kv_len / q_len None, above their range and negative; the rows behind a length and the pitch gap under two random fills;
  * the 4-wave and 16-wave kernels in a child process each (tests/attn_extend_child.py); a captured step replayed while kv_len and q_len move;
  * speculative decoding end to end on RaggedInt8KVCache and PagedInt8KVCache: append, extend, rewind against a plain run of the accepted tokens;
  * the gates: one extend launch of Sq = 4 beats the cheapest route there was, four decode launches on copies of the q slices."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_decode_ref as R
import attn_extend_child as CH
import attn_extend_ref as X
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, medians_us

pytestmark = pytest.mark.gpu
DEV = CH.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dev, _run = CH.dev, CH.run
SIGNED = [(ci, sign) for ci in range(len(X.CASES)) for sign in X.SIGNS]


@pytest.mark.parametrize("case", [1, 4, 3], ids=["kv2x4d128", "kv3x2d80", "kv1x16d64-chunked"])
def test_i1_one_token_is_the_decode_entry(case):
    """Sq = 1, q_len NULL: every output byte equals asq_attn_decode_i8's with the same arguments, at every length of the case (0 keys included)"""
    import attn_decode_child as DC
    qn, kn, vn, lengths = R.operands(case)
    assert R.chunked(case) == (case == 3)
    q, k, v = _dev(qn, kn, vn)
    ml = R.max_len(lengths)
    for sign in X.SIGNS:
        for pv in R.PV_ALPHAS:
            alpha = sign * R.qk_alpha(case, 1)
            want = DC.run(q, k, v, lengths, alpha, pv, ml)
            got = _run(q.unsqueeze(1), k, v, lengths, None, alpha, pv, ml)
            assert_bits_equal(got[:, 0], want, f"(I1) {R.param_id((case, 1))}, qk_alpha {alpha:+.5f}, pv_alpha {pv:.5f}")


@pytest.mark.parametrize("case,sign", SIGNED, ids=[X.param_id((ci, 1, sign)) for ci, sign in SIGNED])
def test_i2_the_single_token_entry_on_the_same_tile_rows(case, sign):
    """(I2) on every case, one-pass and chunked; (I3) as well where nothing is chunked"""
    CH.identity_i2(case, 1, sign, with_i3=not X.chunked(case))


@pytest.mark.parametrize("p", X.PARAMS, ids=[X.param_id(p) for p in X.PARAMS])
def test_cases_by_the_interval_rule(p):
    CH.interval_case(*p)


@pytest.mark.parametrize("i", range(len(X.UNIFORM)), ids=[f"kv{s[0]}x{s[1]}s{s[2]}d{s[3]}" for s in X.UNIFORM])
def test_uniform_staircase_is_exact(i):
    CH.uniform_staircase(i)


@pytest.mark.parametrize("i", range(len(X.STAIRS)), ids=[f"kv{s[0]}x{s[1]}s{s[2]}d{s[3]}" for s in X.STAIRS])
def test_poisoned_staircase_is_exact(i):
    CH.poisoned_staircase(i)


def test_kv_len_and_q_len_none_out_of_range_and_negative():
    case = 1
    hkv, r, sq, d, lengths, _ = X.CASES[case]
    qn, kn, vn = X.operands(case)
    q, k, v = _dev(qn, kn, vn)
    ml, alpha, pv = X.max_len(lengths), X.qk_alpha(case, 1), X.PV_ALPHAS[0]
    B = len(lengths)
    a = _run(q, k, v, None, None, alpha, pv, ml)
    assert_bits_equal(a, _run(q, k, v, [ml] * B, [sq] * B, alpha, pv, ml), "kv_len and q_len None against max_len and Sq")
    s_lo, s_hi, _, _ = X.expanded_sums(qn, kn, vn, X.row_keys([ml] * B, None, sq, ml), alpha)
    R.check(a, *R.interval(s_lo, s_hi, pv), "kv_len and q_len None")
    wild_n, wild_m = [ml + 1, -5, lengths[2], 1 << 30], [7, 2, -3, 1 << 30]
    clamped_n, clamped_m = [ml, 0, lengths[2], ml], [sq, 2, 0, sq]
    got = _run(q, k, v, wild_n, wild_m, alpha, pv, ml)
    assert_bits_equal(got, _run(q, k, v, clamped_n, clamped_m, alpha, pv, ml), "kv_len / q_len outside their range against their clamped values")
    L = X.row_keys(wild_n, wild_m, sq, ml)
    assert L.tolist() == X.row_keys(clamped_n, clamped_m, sq, ml).tolist() and not got[L == 0].any() and (L[1] == 0).all() and (L[2] == 0).all()
    s_lo, s_hi, _, _ = X.expanded_sums(qn, kn, vn, L, alpha)
    R.check(got, *R.interval(s_lo, s_hi, pv), "clamped kv_len / q_len")
    # q_len alone, kv_len alone
    assert_bits_equal(_run(q, k, v, None, [1, 2, 3, 4], alpha, pv, ml), _run(q, k, v, [ml] * B, [1, 2, 3, 4], alpha, pv, ml), "kv_len None with a q_len")
    assert_bits_equal(_run(q, k, v, lengths, None, alpha, pv, ml), _run(q, k, v, lengths, [sq] * B, alpha, pv, ml), "q_len None with a kv_len")


@pytest.mark.parametrize("case", [1, 2, 4])
def test_rows_behind_the_length_and_the_pitch_gap_do_not_matter(case):
    hkv, r, sq, d, lengths, q_len = X.CASES[case]
    qn, kn, vn = X.operands(case)
    ml = X.max_len(lengths)
    outs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        k2, v2 = kn.copy(), vn.copy()
        for b, n in enumerate(lengths):
            k2[b, n:] = rng.integers(-128, 128, k2[b, n:].shape, dtype=np.int8)
            v2[b, n:] = rng.integers(-128, 128, v2[b, n:].shape, dtype=np.int8)
        q, k, v = _dev(qn, k2, v2)
        outs.append(_run(q, k, v, lengths, q_len, X.qk_alpha(case, 1), X.PV_ALPHAS[0], ml))
    assert_bits_equal(outs[0], outs[1], f"case {case + 1}: the output depends on rows >= n_b")


@pytest.mark.parametrize("nw", [4, 16])
def test_the_4_wave_and_16_wave_kernels_in_a_child_process(nw):
    """ASQ_DECODE_WAVES is latched on first use: tests/attn_extend_child.py runs (I2) on cases 3 and 5 and the two staircases in a fresh process.  A child that ends by a
    signal or the time limit fails this test; nothing is tried again"""
    env = dict(os.environ, ASQ_DECODE_WAVES=str(nw))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_extend_child.py"), str(nw)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"the {nw}-wave child returned {r.returncode}: {r.stdout[-1500:]} {r.stderr[-1500:]}"
    assert f"{nw} waves: all passed" in r.stdout


def test_a_captured_step_replays_as_kv_len_and_q_len_move():
    """one launch under torch.cuda.graph; kv_len and q_len are rewritten in place between the replays and each replay equals the eager call"""
    case = 3
    hkv, r, sq, d, lengths, _ = X.CASES[case]
    qn, kn, vn = X.operands(case)
    q, k, v = _dev(qn, kn, vn)
    ml, alpha, pv = X.max_len(lengths), X.qk_alpha(case, 1), X.PV_ALPHAS[0]
    moves = [([3, 255, 2049], [3, 2, 3]), ([10, 1025, 100], [1, 3, 0]), ([ml, 0, 1024], [3, 3, 2])]
    n, m = (torch.tensor(x, dtype=torch.int32, device=DEV) for x in moves[0])
    ops.attn_extend_i8(q, k[:, :ml], v[:, :ml], n, alpha, pv, q_len=m)          # (the first call sets the kernel's LDS attribute: not inside a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.attn_extend_i8(q, k[:, :ml], v[:, :ml], n, alpha, pv, q_len=m)
    outs = []
    for kv, ql in moves:
        n.copy_(torch.tensor(kv, dtype=torch.int32)), m.copy_(torch.tensor(ql, dtype=torch.int32))
        graph.replay()
        outs.append(out.clone())
    torch.cuda.synchronize()
    for (kv, ql), got in zip(moves, outs):
        assert_bits_equal(got.cpu().numpy(), _run(q, k, v, kv, ql, alpha, pv, ml), f"the replay with kv_len {kv}, q_len {ql} differs from the eager call")
    assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[1], outs[2])


def _tables(T, D, dt):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().to(dt).to(DEV), ang.sin().to(dt).to(DEV)


@pytest.mark.parametrize("paged", [False, True], ids=["ragged", "paged16"])
def test_speculative_steps_end_to_end(paged):
    """B = 3, 4 / 2 heads of d = 64: a padded prefill of 5 / 12 / 9 tokens, then three steps of Sq = 4 draft tokens -- append, extend, rewind(4 - accepted) -- against a
    plain run that feeds only the accepted tokens one at a time through the append and decode that were there before.  After every step each sequence's cache rows
    0 .. n_b - 1 are byte-equal, and every accepted token's attention output is decode's, byte for byte (all lengths are one-pass: (I3))."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, PagedInt8KVCache, RaggedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, smax, prompts, Sq = 3, 4, 2, 64, 32, [5, 12, 9], 4
    accepted = [[1, 4, 2], [3, 2, 4], [4, 1, 3]]
    qs, ks, vs = 0.037, 0.011, 0.073
    dt = torch.float16
    g = torch.Generator().manual_seed(53500)
    cos, sin = _tables(smax, D, dt)
    mod = RopeQuantQKV(qs, ks, vs).to(DEV)
    att = Int8Attention.from_scale(qs, ks, vs, 0.05, sm_scale=D ** -0.5, causal=True).to(DEV)
    spec = PagedInt8KVCache(8, 16, Hkv, D, B, smax, device=DEV) if paged else RaggedInt8KVCache(B, smax, Hkv, D, device=DEV)
    plain = RaggedInt8KVCache(B, smax, Hkv, D, device=DEV)

    def draw(S):
        fused = (torch.randn((B, S, (Hq + 2 * Hkv) * D), generator=g) * 2).to(dt).to(DEV)
        return [fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv))]

    def same_rows(what):
        assert spec.lengths == plain.lengths and spec.kv_len.tolist() == plain.kv_len.tolist() == plain.lengths, what
        for b, n in enumerate(plain.lengths):
            sk, sv = spec.gather(b) if paged else (spec.k[b, :n], spec.v[b, :n])
            assert torch.equal(sk, plain.k[b, :n]) and torch.equal(sv, plain.v[b, :n]), f"{what}, sequence {b}: cache rows differ from the plain run's"

    q, k, v = draw(max(prompts))
    mod(q, k, v, cos, sin, cache=spec, advance=prompts)
    mod(q, k, v, cos, sin, cache=plain, advance=prompts)
    same_rows("prefill")
    for step, acc in enumerate(accepted):
        q, k, v = draw(Sq)
        q8, kc, vc = mod(q, k, v, cos, sin, cache=spec)
        if paged:
            out = att.extend_paged(q8, kc, vc, spec.block_table, spec.kv_len, max_len=smax)
            held = [len(pg) for pg in spec.pages]
        else:
            out = att.extend(q8, kc, vc, spec.kv_len, max_len=spec.bound())
        assert tuple(out.shape) == (B, Sq, Hq, D) and int(out.abs().max()) > 10          # the scales leave a signal
        spec.rewind([Sq - a for a in acc])
        if paged:
            assert [len(pg) for pg in spec.pages] == [-(-n // 16) for n in spec.lengths] and all(a <= h for a, h in zip([len(pg) for pg in spec.pages], held))
            assert sorted([p for pg in spec.pages for p in pg] + spec.free) == list(range(8))
        for j in range(Sq):
            live = [1 if j < a else 0 for a in acc]
            q8_1, _, _ = mod(q[:, j:j + 1], k[:, j:j + 1], v[:, j:j + 1], cos, sin, cache=plain, advance=live)
            one = att.decode(q8_1, plain.k, plain.v, plain.kv_len, max_len=plain.bound())
            for b in range(B):
                if live[b]:
                    assert torch.equal(q8_1[b], q8[b, j:j + 1]), f"step {step}, sequence {b}, token {j}: q8 differs"
                    assert torch.equal(one[b, 0], out[b, j]), f"step {step}, sequence {b}, token {j}: extend's output is not decode's"
        same_rows(f"step {step}")
    assert plain.lengths == [p + sum(a[b] for a in accepted) for b, p in enumerate(prompts)]


def _gate(paged):
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, Hq, Hkv, D, smax, n, Sq, nrot, P = 16, 32, 8, 128, 4352, 4096, 4, 5, 16
    att = Int8Attention(R.SR.alphas((1, 1, D))[1], 1.0 / 127, causal=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(53600 + paged)
    lens = [torch.full((B,), n - (Sq - 1 - s), dtype=torch.int32, device=DEV) for s in range(Sq)]
    sets = []
    for _ in range(nrot):      # 5 x 2 x 67 .. 73 MB; candidate j of iteration i takes set (i + 2 j) mod 5: what a call reads was last touched five calls earlier
        q = torch.randint(-128, 128, (B, Sq, Hq, D), dtype=torch.int8, device=DEV, generator=g)
        if paged:
            k, v = (torch.randint(-128, 128, (B * n // P, P, Hkv, D), dtype=torch.int8, device=DEV, generator=g) for _ in range(2))
            tab = torch.randperm(B * n // P, generator=torch.Generator().manual_seed(53610)).to(torch.int32).view(B, n // P).to(DEV)
        else:
            k, v = (torch.randint(-128, 128, (B, smax, Hkv, D), dtype=torch.int8, device=DEV, generator=g) for _ in range(2))
            tab = None
        sets.append((q, k, v, tab, q[:, :1].contiguous()))
    if paged:
        new = lambda i: att.extend_paged(sets[i][0], sets[i][1], sets[i][2], sets[i][3], lens[-1], max_len=n)  # noqa: E731
        one = lambda i, s, q1: att.decode_paged(q1, sets[i][1], sets[i][2], sets[i][3], lens[s], max_len=n)  # noqa: E731
    else:
        new = lambda i: att.extend(sets[i][0], sets[i][1], sets[i][2], lens[-1], max_len=n)  # noqa: E731
        one = lambda i, s, q1: att.decode(q1, sets[i][1], sets[i][2], lens[s], max_len=n)  # noqa: E731
    old = lambda i: [one(i, s, sets[i][0][:, s:s + 1].contiguous()) for s in range(Sq)]  # noqa: E731
    plain = lambda i: one(i, Sq - 1, sets[i][4])  # noqa: E731
    got, want = new(0), old(0)
    sure = 0
    for s in range(Sq):          # the two routes agree wherever the chunk (1024 keys at R = 16, 4096 at r = 4) cannot matter: compared loosely here, the identities are above
        sure += int((got[:, s:s + 1] == want[s]).sum())
    assert sure > 0.9 * got.numel(), f"the two routes agree on {sure} of {got.numel()} outputs only"
    ta, tb, tc = medians_us([lambda i, f=f, j=j: f((i + 2 * j) % nrot) for j, f in enumerate((new, old, plain))], nrot)
    name = "extend_paged (page 16)" if paged else "extend"
    print(f"{name} in place {ta:.1f} us, four decode launches on copies of the q slices {tb:.1f} us, one plain decode launch {tc:.1f} us: "
          f"new / one decode = {ta / tc:.2f}, four decodes / new = {tb / ta:.2f}")
    assert ta < tb, f"the {name} launch ({ta:.1f} us) is not faster than four decode launches on copies of the q slices ({tb:.1f} us)"


def test_gate_faster_than_four_decode_launches():
    """16 sequences x 32 / 8 heads x d = 128, 4096 keys, Sq = 4: (a) the extend launch on the cache in place against (b) the cheapest route there was, four
    Int8Attention.decode calls, each on a contiguous copy of q8[:, s] with its own kv_len - (3 - s); (c) one plain decode launch is printed for the ratio"""
    _gate(False)


def test_gate_paged_faster_than_four_decode_launches():
    """the same comparison through extend_paged / decode_paged at page 16, the pages of all sequences scattered over the pool"""
    _gate(True)
