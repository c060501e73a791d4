"""GPU: asq_attn_decode_i8 through ops.attn_decode_i8 / Int8Attention.decode (include/asq_hip_decode.h).

  * every case of tests/attn_decode_ref.py by its interval rule, within its caps: ceil(D / 64) of 1 to 4, each on the one-pass and on the chunked path, r that are no
    powers of two; the second group's chunked cases under -qk_alpha as well (the min reference moving between chunks);
  * constructed families that are exact by design, bit for bit: uniform softmax; one-hot, also once per r = 1 .. 16 and once per D = 16 .. 256 (head mapping,
    lengths, addressing, epilogue); the key-position walk (one weight per sequence on every seam of the loops: tile, K step, wave strides, chunk edges, last partial
    tile); two weights in different chunks under both signs (the rescale, exactly: 34 v[A] + 93 v[B]);
  * the rows behind a sequence's length and the pitch gap under two random fills, and poisoned with the key that would win a row: the outputs must not move;
  * the 4-wave and 16-wave kernels (ASQ_DECODE_WAVES is read once per process) in a child process each: tests/attn_decode_child.py;
  * kv_len None / above max_len / negative, a negative qk_alpha;
  * against Int8Attention.forward(layout="bshd") on contiguous copies; a ragged prefill + three decode steps end to end against single-sequence runs;
  * the gate: at the bench shape the launch on the cache in place beats what a B > 1 caller paid before (two copies + the two-launch forward)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_decode_child as CH
import attn_decode_ref as R
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, medians_us, ref_out

pytestmark = pytest.mark.gpu
DEV = CH.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dev, _run = CH.dev, CH.run       # (the device runs that the wave children repeat live in tests/attn_decode_child.py)


@pytest.mark.parametrize("p", R.PARAMS, ids=[R.param_id(p) for p in R.PARAMS])
def test_cases_by_the_interval_rule(p):
    CH.interval_case(*p)


@pytest.mark.parametrize("p", R.NEG_PARAMS, ids=[R.param_id(p) for p in R.NEG_PARAMS])
def test_chunked_cases_by_the_interval_rule_with_a_negative_alpha(p):
    """the reference is the smallest score and a later chunk moves it down: the caps re-derived for the sign, then the interval rule"""
    CH.interval_case(*p, sign=-1)


def test_uniform_softmax_is_exact():
    qn, kn, vn, lengths, alpha, ml = R.uniform_case()
    q, k, v = _dev(qn, kn, vn)
    r = qn.shape[1] // kn.shape[2]
    s = np.stack([vn[b, :n].astype(np.int64).sum(axis=0) for b, n in enumerate(lengths)]).repeat(r, axis=1)      # every p = 1: sum v, the same for the r heads of a group
    for pv in (1.0 / 127, 0.01, 1.0):
        assert_bits_equal(_run(q, k, v, lengths, alpha, pv, ml), ref_out(s, torch.int8, pv), f"uniform softmax, pv_alpha {pv}")
    s_lo, s_hi, nband, _ = R.sums(qn, kn, vn, lengths, alpha)
    assert nband == 0 and np.array_equal(s_lo, s) and np.array_equal(s_hi, s)


@pytest.mark.parametrize("i", range(len(R.ONE_HOT)))
def test_one_hot_softmax_is_exact(i):
    CH.one_hot(R.one_hot_case(i), f"one-hot {R.ONE_HOT[i]}")


@pytest.mark.parametrize("i", range(len(R.ONE_HOT_R)), ids=[f"r{s[1]}" for s in R.ONE_HOT_R])
def test_one_hot_at_every_r(i):
    """rows t16 < r of the tile, the head mapping and the [r][chunk + 4] strip pitch at every r the entry takes"""
    CH.one_hot(R.one_hot_r_case(i), f"one-hot {R.ONE_HOT_R[i]}")


@pytest.mark.parametrize("i", range(len(R.ONE_HOT_D)), ids=[f"d{s[2]}" for s in R.ONE_HOT_D])
def test_one_hot_at_every_head_dim(i):
    """columns col < D of the last 64-column block, the addressing and the epilogue at every D the entry takes"""
    CH.one_hot(R.one_hot_d_case(i), f"one-hot {R.ONE_HOT_D[i]}")


@pytest.mark.parametrize("i", range(len(R.WALK)), ids=[f"kv{s[0]}x{s[1]}d{s[2]}" for s in R.WALK])
def test_key_position_walk_is_exact(i):
    """every key counted exactly once, at the seams: three chunks, sequence b's only weight at the b-th of walk_positions(); one launch per shape"""
    CH.walk(i, 8)


@pytest.mark.parametrize("neg", [False, True], ids=["max", "min"])
@pytest.mark.parametrize("i", range(len(R.WALK)), ids=[f"kv{s[0]}x{s[1]}d{s[2]}" for s in R.WALK])
def test_two_weights_in_different_chunks_are_exact(i, neg):
    """the rescale of pass 1, exactly: 34 v[A] + 93 v[B] whichever chunk holds which, for the max reference and (-qk_alpha on negated keys) the min reference"""
    CH.two_weights(i, neg)


@pytest.mark.parametrize("case", [1, 3, 4])
def test_rows_behind_the_length_and_the_pitch_gap_do_not_matter(case):
    qn, kn, vn, lengths = R.operands(case)
    ml = R.max_len(lengths)
    outs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        k2, v2 = kn.copy(), vn.copy()
        for b, n in enumerate(lengths):
            k2[b, n:] = rng.integers(-128, 128, k2[b, n:].shape, dtype=np.int8)
            v2[b, n:] = rng.integers(-128, 128, v2[b, n:].shape, dtype=np.int8)
        q, k, v = _dev(qn, k2, v2)
        outs.append(_run(q, k, v, lengths, R.qk_alpha(case, 1), R.PV_ALPHAS[0], ml))
    assert_bits_equal(outs[0], outs[1], f"case {case}: the output depends on rows >= n_b")


@pytest.mark.parametrize("case", R.POISONED, ids=[R.param_id((c, 1)) for c in R.POISONED])
def test_a_poisoned_tail_does_not_matter(case):
    """every row at or beyond n_b, the rows between max_len and the pitch included, holds the key that would win a row outright and V of +-127; kv_len[0] is above
    max_len, so the poison sits exactly at row max_len.  One stray key moves most outputs: bit-equal to the run with those rows zeroed, and inside the intervals"""
    qn = R.operands(case)[0]
    k2, v2, k0, v0, kv_len, n_b = R.poisoned(case)
    ml, alpha, pv = R.max_len(R.CASES[case][3]), R.qk_alpha(case, 1), R.PV_ALPHAS[0]
    n = torch.tensor(kv_len, dtype=torch.int32, device=DEV)
    q, kp, vp, kz, vz = _dev(qn, k2, v2, k0, v0)
    got = _run(q, kp, vp, None, alpha, pv, ml, kv_len=n)
    assert_bits_equal(got, _run(q, kz, vz, None, alpha, pv, ml, kv_len=n), f"case {case}: the output depends on rows >= n_b")
    s_lo, s_hi, nband, total = R.poisoned_sums(case)
    lo, hi = R.interval(s_lo, s_hi, pv)
    R.caps(lo, hi, nband, total, f"poisoned case {case}")
    R.check(got, lo, hi, f"poisoned case {case}")


@pytest.mark.parametrize("nw", [4, 16])
def test_the_4_wave_and_16_wave_kernels_in_a_child_process(nw):
    """ASQ_DECODE_WAVES is latched on first use: tests/attn_decode_child.py runs the walk for its own number of waves, the two weights and three interval cases in a
    fresh process.  A child that ends by a signal or the time limit fails this test; nothing is tried again"""
    env = dict(os.environ, ASQ_DECODE_WAVES=str(nw))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_decode_child.py"), str(nw)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"the {nw}-wave child returned {r.returncode}: {r.stdout[-1500:]} {r.stderr[-1500:]}"
    assert f"{nw} waves: all passed" in r.stdout


def test_kv_len_variations_and_a_negative_alpha():
    case, si = 2, 1
    qn, kn, vn, lengths = R.operands(case)
    q, k, v = _dev(qn, kn, vn)
    ml, alpha, pv = R.max_len(lengths), R.qk_alpha(case, si), R.PV_ALPHAS[0]
    full = (ml,) * len(lengths)
    a = _run(q, k, v, full, alpha, pv, ml, kv_len=None)
    assert_bits_equal(a, _run(q, k, v, full, alpha, pv, ml), "kv_len None against kv_len = max_len")
    s_lo, s_hi, _, _ = R.sums(qn, kn, vn, full, alpha)
    R.check(a, *R.interval(s_lo, s_hi, pv), "kv_len None")
    wild = torch.tensor([ml + 1, -5, lengths[2], 1 << 30, -(1 << 31)], dtype=torch.int32, device=DEV)
    clamped = [ml, 0, lengths[2], ml, 0]
    got = _run(q, k, v, None, alpha, pv, ml, kv_len=wild)
    assert_bits_equal(got, _run(q, k, v, clamped, alpha, pv, ml), "kv_len outside 0 .. max_len against its clamped value")
    assert not got[1].any() and not got[4].any()
    q4 = q.view(q.shape[0], 1, q.shape[1], q.shape[2])          # [B, 1, Hq, D] in, the same shape out, the same bytes
    out4 = ops.attn_decode_i8(q4, k[:, :ml], v[:, :ml], torch.tensor(lengths, dtype=torch.int32, device=DEV), alpha, pv)
    assert out4.shape == q4.shape and np.array_equal(out4.cpu().numpy().reshape(qn.shape), _run(q, k, v, lengths, alpha, pv, ml))
    # a negative qk_alpha: the reference is the smallest score
    s_lo, s_hi, nband, total = R.sums(qn, kn, vn, lengths, -alpha)
    lo, hi = R.interval(s_lo, s_hi, pv)
    R.caps(lo, hi, nband, total, "negative qk_alpha")
    R.check(_run(q, k, v, lengths, -alpha, pv, ml), lo, hi, "negative qk_alpha")


@pytest.mark.parametrize("B", [1, 3])
def test_against_the_two_launch_forward_on_contiguous_copies(B):
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    hkv, r, d, n = 2, 4, 128, 777
    rng = np.random.default_rng(52400 + B)
    qn = rng.integers(-128, 128, (B, hkv * r, d), dtype=np.int8)
    kn, vn = (rng.integers(-128, 128, (B, n + 5, hkv, d), dtype=np.int8) for _ in range(2))
    alpha, pv = R.SR.alphas((1, 1, d))[1], R.PV_ALPHAS[0]
    att = Int8Attention(alpha, pv, causal=True).to(DEV)
    q, k, v = _dev(qn, kn, vn)
    new = att.decode(q.view(B, 1, hkv * r, d), k[:, :n], v[:, :n]).cpu().numpy().reshape(qn.shape)
    old = att(q.view(B, 1, hkv * r, d), k[:, :n].contiguous(), v[:, :n].contiguous(), layout="bshd").cpu().numpy().reshape(qn.shape)
    s_lo, s_hi, nband, total = R.sums(qn, kn, vn, (n,) * B, att.qk_bmm._alpha())
    lo, hi = R.interval(s_lo, s_hi, att.pv_bmm._alpha())
    R.caps(lo, hi, nband, total, f"B={B}")
    R.check(new, lo, hi, f"decode, B={B}")
    R.check(old, lo, hi, f"two-launch forward, B={B}")
    sure = lo == hi
    print(f"B={B}: {int((new != old).sum())} of {new.size} outputs differ between the two paths, {int((~sure).sum())} have lo != hi")
    assert np.array_equal(new[sure], old[sure])


def _tables(T, D, dt):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))
    ang = torch.arange(T, dtype=torch.float32)[:, None] * inv[None, :]
    return ang.cos().to(dt).to(DEV), ang.sin().to(dt).to(DEV)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_ragged_prefill_and_decode_end_to_end(dt):
    """B = 3, prompts of 5 / 12 / 9 tokens as one padded prefill, then three single-token steps; 4 / 2 heads of d = 64.  After every step each sequence's cache rows
    0 .. n_b - 1 and its q8 are byte-equal to a single-sequence Int8KVCache + RopeQuantQKV run over the same tokens at the same positions, and Int8Attention.decode
    passes the interval rule on the cache's bytes."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, Int8KVCache, RaggedInt8KVCache, RopeQuantQKV
    B, Hq, Hkv, D, smax, prompts = 3, 4, 2, 64, 20, [5, 12, 9]
    qs, ks, vs = 0.037, 0.011, 0.073
    g = torch.Generator().manual_seed(52500)
    cos, sin = _tables(smax, D, dt)
    mod = RopeQuantQKV(qs, ks, vs).to(DEV)
    att = Int8Attention.from_scale(qs, ks, vs, 0.05, sm_scale=D ** -0.5, causal=True).to(DEV)
    cache = RaggedInt8KVCache(B, smax, Hkv, D, device=DEV)
    singles = [Int8KVCache(1, smax, Hkv, D, device=DEV) for _ in range(B)]
    for step, S in enumerate((max(prompts), 1, 1, 1)):
        fused = (torch.randn((B, S, (Hq + 2 * Hkv) * D), generator=g) * 2).to(dt).to(DEV)
        q, k, v = (fused[..., a * D:b * D].unflatten(-1, (-1, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))
        true = prompts if step == 0 else [1] * B
        q8, kc, vc = mod(q, k, v, cos, sin, cache=cache, advance=true if step == 0 else None)
        assert kc.data_ptr() == cache.k.data_ptr() and vc.data_ptr() == cache.v.data_ptr() and tuple(q8.shape) == (B, S, Hq, D)
        for b in range(B):
            t = true[b]
            q8_1, k8_1, v8_1 = mod(q[b:b + 1, :t], k[b:b + 1, :t], v[b:b + 1, :t], cos, sin, cache=singles[b])
            n = singles[b].length
            assert cache.lengths[b] == n
            assert torch.equal(q8[b:b + 1, :t], q8_1), f"step {step}, sequence {b}: q8 differs from the single-sequence run"
            assert torch.equal(cache.k[b:b + 1, :n], k8_1) and torch.equal(cache.v[b:b + 1, :n], v8_1), f"step {step}, sequence {b}: cache rows differ"
        assert cache.kv_len.tolist() == cache.lengths
        if S == 1:
            out = att.decode(q8, cache.k, cache.v, cache.kv_len, max_len=cache.bound())
            assert tuple(out.shape) == (B, 1, Hq, D)
            qn, kn, vn = q8.view(B, Hq, D).cpu().numpy(), cache.k.cpu().numpy(), cache.v.cpu().numpy()
            s_lo, s_hi, _, _ = R.sums(qn, kn, vn, tuple(cache.lengths), att.qk_bmm._alpha())
            lo, hi = R.interval(s_lo, s_hi, att.pv_bmm._alpha())
            R.check(out.view(B, Hq, D).cpu().numpy(), lo, hi, f"step {step}")
            assert int(out.abs().max()) > 10                    # the scales leave a signal
            assert torch.equal(out, att.decode(q8, cache.k, cache.v, cache.kv_len))       # the capacity as the bound: the same bytes


def test_gate_faster_than_copies_plus_the_two_launch_forward():
    """16 sequences x 32 / 8 heads x d = 128 in caches of Smax = 4352, all lengths 4096: (a) the new launch on the cache in place against (b) contiguous() of both
    views + Int8Attention.forward(layout="bshd"), what a B > 1 caller paid before.  (a) / (c), the forward alone on copies made outside the timer, is printed."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, Hq, Hkv, D, smax, n, nrot = 16, 32, 8, 128, 4352, 4096, 3
    att = Int8Attention(R.SR.alphas((1, 1, D))[1], 1.0 / 127, causal=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(52600)
    sets = []
    for _ in range(nrot):      # 3 x 2 x 73 MB: the rotation walks past the Infinity Cache
        q = torch.randint(-128, 128, (B, 1, Hq, D), dtype=torch.int8, device=DEV, generator=g)
        k, v = (torch.randint(-128, 128, (B, smax, Hkv, D), dtype=torch.int8, device=DEV, generator=g) for _ in range(2))
        sets.append((q, k, v, k[:, :n].contiguous(), v[:, :n].contiguous(), torch.full((B,), n, dtype=torch.int32, device=DEV)))
    a = lambda i: att.decode(sets[i][0], sets[i][1], sets[i][2], sets[i][5], max_len=n)  # noqa: E731
    b = lambda i: att(sets[i][0], sets[i][1][:, :n].contiguous(), sets[i][2][:, :n].contiguous(), layout="bshd")  # noqa: E731
    c = lambda i: att(sets[i][0], sets[i][3], sets[i][4], layout="bshd")  # noqa: E731
    ta, tb, tc = medians_us([a, b, c], nrot)
    print(f"decode in place {ta:.1f} us, copies + two-launch forward {tb:.1f} us, two-launch forward alone {tc:.1f} us: a / c = {ta / tc:.2f}")
    assert ta < tb, f"the decode launch ({ta:.1f} us) is not faster than the copies + the two-launch forward ({tb:.1f} us)"
