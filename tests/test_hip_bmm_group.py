"""GPU: the batched int8 matmuls with a shared b (ASQ_BMM_B_GROUP(r) on asq_bmm_i8's out_kind, `b_group=r` on ops.bmm_i8 / bmm_i8_kn / bmm_i8_softmax_q8:
b holds batch / r entries and entry i uses b[i // r]) and Int8Attention's grouped-query routes on top of them.

The grouped call is the base kind's kernel with another address for b, so the first yardstick is the base kind itself on b.repeat_interleave(r, 0), bit
for bit, on every kernel form: "m16" / "t128" / "m16kn" / "t128kn" on their byte and 16-B load paths, with two column tiles and a row tail, and "sm128"
full and causal.  The second is independent of the library: an int64 einsum over b[i // r] in numpy, then bmm_ref.ref_out (plain kinds) or
softmax_q8_ref's target and acceptance rule with its own BAND_CAP (softmax kinds)."""
import numpy as np
import pytest
import torch

import softmax_q8_ref as R
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, medians_us, ref_out, tbits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (torch.int32, torch.float32, torch.int8)
ALPHA = 0.0123

# (batch, r, M, N, K)
PLAIN = [(6, 3, 5, 33, 70), (8, 4, 16, 48, 64), (4, 2, 40, 130, 129), (8, 4, 130, 256, 128)]
SOFTMAX = [(8, 4, 130, 130, 64), (6, 3, 3, 200, 72), (4, 2, 200, 70, 16), (4, 2, 5, 7, 0)]        # (4, 2, 200, 70, 16): causal rows without a visible key
ident = lambda s: "x".join(map(str, s))


def operands(shape, kn=False):
    """int8 a [batch, M, K] and the SMALL b, [batch / r, N, K] or (kn) [batch / r, K, N], as numpy arrays"""
    B, r, M, N, K = shape
    rng = np.random.default_rng(9000 + 1000 * B + 100 * r + M + 7 * N + 13 * K + kn)
    return rng.integers(-128, 128, (B, M, K), dtype=np.int8), rng.integers(-128, 128, (B // r, K, N) if kn else (B // r, N, K), dtype=np.int8)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def softmax_alpha(K):
    """a score standard deviation of about 4 (softmax_q8_ref.alphas)"""
    return float(np.float32(4.0 / (5461.0 * np.sqrt(max(K, 1)))))


def acc_grouped(a, b, r, kn):
    """[batch, M, N] int64 = a[i] . b[i // r] exactly"""
    return np.einsum("bmk,bkn->bmn" if kn else "bmk,bnk->bmn", a.astype(np.int64), b.astype(np.int64)[np.arange(a.shape[0]) // r])


@pytest.mark.parametrize("kn", [False, True], ids=["nk", "kn"])
@pytest.mark.parametrize("shape", PLAIN, ids=ident)
def test_grouped_call_is_the_base_kind_on_the_expanded_b(shape, kn):
    B, r, M, N, K = shape
    a, b = map(dev, operands(shape, kn))
    op = ops.bmm_i8_kn if kn else ops.bmm_i8
    b_all = b.repeat_interleave(r, 0)
    assert b_all.shape[0] == B and b.shape[0] * r == B
    for kind in KINDS:
        got = op(a, b, kind, ALPHA, b_group=r)
        want = op(a, b_all, kind, ALPHA)
        assert got.dtype == kind and tuple(got.shape) == (B, M, N) and got.is_contiguous()
        assert torch.equal(tbits(got), tbits(want)), f"{kind} {shape} kn={kn}: differs from the call on the expanded b"
        code = ops._BMM_KIND[kind] | (L.ASQ_BMM_B_KN if kn else 0)
        name = ops.bmm_kernel_name(B, M, N, K, code | L.ASQ_BMM_B_GROUP(r))
        assert name == ops.bmm_kernel_name(B, M, N, K, code) == ("m16" if M <= 16 else "t128") + ("kn" if kn else "")
    assert int(want.abs().max()) > 0


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("shape", SOFTMAX, ids=ident)
def test_grouped_softmax_is_the_base_kind_on_the_expanded_b(shape, causal):
    B, r, M, N, K = shape
    a, b = map(dev, operands(shape))
    alpha = softmax_alpha(K)
    got = ops.bmm_i8_softmax_q8(a, b, alpha, causal, b_group=r)
    want = ops.bmm_i8_softmax_q8(a, b.repeat_interleave(r, 0), alpha, causal)
    assert got.dtype == torch.int8 and tuple(got.shape) == (B, M, N)
    assert torch.equal(got, want), f"{shape} causal={causal}: differs from the call on the expanded b"
    assert int(want.max()) > 0
    code = 18 | (L.ASQ_BMM_CAUSAL if causal else 0)
    assert ops.bmm_kernel_name(B, M, N, K, code | L.ASQ_BMM_B_GROUP(r)) == "sm128"
    if causal and M > N:
        assert not got[:, :M - N].any() and got[:, M - N].any()


def test_one_b_for_the_whole_batch():
    """r == batch"""
    for shape in ((5, 5, 7, 40, 48), (3, 3, 50, 130, 100)):
        B, r, M, N, K = shape
        for kn in (False, True):
            a, b = map(dev, operands(shape, kn))
            assert b.shape[0] == 1
            op = ops.bmm_i8_kn if kn else ops.bmm_i8
            for kind in KINDS:
                assert torch.equal(tbits(op(a, b, kind, ALPHA, b_group=r)), tbits(op(a, b.expand(B, -1, -1).contiguous(), kind, ALPHA)))
        a, b = map(dev, operands(shape))
        for causal in (False, True):
            assert torch.equal(ops.bmm_i8_softmax_q8(a, b, softmax_alpha(K), causal, b_group=r),
                               ops.bmm_i8_softmax_q8(a, b.expand(B, -1, -1).contiguous(), softmax_alpha(K), causal))


def test_explicit_group_of_one_is_the_plain_call():
    shape = (3, 1, 20, 40, 48)
    a, b = map(dev, operands(shape))
    b_kn = b.transpose(1, 2).contiguous()
    for kind in KINDS:
        assert torch.equal(tbits(ops.bmm_i8(a, b, kind, ALPHA, b_group=1)), tbits(ops.bmm_i8(a, b, kind, ALPHA)))
        assert torch.equal(tbits(ops.bmm_i8_kn(a, b_kn, kind, ALPHA, b_group=1)), tbits(ops.bmm_i8_kn(a, b_kn, kind, ALPHA)))
    for causal in (False, True):
        assert torch.equal(ops.bmm_i8_softmax_q8(a, b, 1e-4, causal, b_group=1), ops.bmm_i8_softmax_q8(a, b, 1e-4, causal))


def test_a_groups_bytes_do_not_depend_on_the_other_groups():
    for shape in ((6, 3, 9, 70, 100), (6, 2, 130, 96, 80)):
        B, r, M, N, K = shape
        for kn in (False, True):
            a, b = map(dev, operands(shape, kn))
            op = ops.bmm_i8_kn if kn else ops.bmm_i8
            for kind in KINDS:
                many = op(a, b, kind, ALPHA, b_group=r)
                assert torch.equal(tbits(many), tbits(op(a, b, kind, ALPHA, b_group=r)))          # deterministic
                for g in range(B // r):
                    one = op(a[g * r:(g + 1) * r].contiguous(), b[g:g + 1].contiguous(), kind, ALPHA, b_group=r)
                    assert torch.equal(tbits(many[g * r:(g + 1) * r]), tbits(one)), (shape, kn, kind, g)
        a, b = map(dev, operands(shape))
        for causal in (False, True):
            many = ops.bmm_i8_softmax_q8(a, b, softmax_alpha(K), causal, b_group=r)
            for g in range(B // r):
                one = ops.bmm_i8_softmax_q8(a[g * r:(g + 1) * r].contiguous(), b[g:g + 1].contiguous(), softmax_alpha(K), causal, b_group=r)
                assert torch.equal(many[g * r:(g + 1) * r], one), (shape, causal, g)


@pytest.mark.parametrize("kn", [False, True], ids=["nk", "kn"])
@pytest.mark.parametrize("shape", [(6, 3, 5, 33, 70), (4, 2, 40, 130, 129)], ids=["m16", "t128"])
def test_plain_kinds_against_numpy(shape, kn):
    B, r, M, N, K = shape
    a, b = operands(shape, kn)
    acc = acc_grouped(a, b, r, kn).astype(np.int32)
    op = ops.bmm_i8_kn if kn else ops.bmm_i8
    for kind in KINDS:
        got = op(dev(a), dev(b), kind, ALPHA, b_group=r)
        assert_bits_equal(got.cpu().numpy(), ref_out(acc, kind, ALPHA), f"{kind} {shape} kn={kn}")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_softmax_kinds_against_numpy(causal):
    shape = (6, 3, 40, 70, 72)
    B, r, M, N, K = shape
    a, b = operands(shape)
    alpha = softmax_alpha(K)
    got = ops.bmm_i8_softmax_q8(dev(a), dev(b), alpha, causal, b_group=r).cpu().numpy()
    assert got.min() >= 0
    R.check(got, R.target(acc_grouped(a, b, r, False), alpha, causal), N, f"{shape} causal={causal}")


def test_bad_groups_raise_before_launch():
    a = torch.zeros((4, 8, 32), dtype=torch.int8, device=DEV)
    b = torch.zeros((2, 16, 32), dtype=torch.int8, device=DEV)
    for r in (1, 3, 4, 0, -2, 257, 2.0, None):
        with pytest.raises(ValueError) as info:
            ops.bmm_i8(a, b, torch.int8, 1.0, b_group=r)
        assert "(4, 8, 32)" in str(info.value) and "(2, 16, 32)" in str(info.value)          # both shapes are named
    with pytest.raises(ValueError):
        ops.bmm_i8_kn(a, b.transpose(1, 2).contiguous()[:1], torch.int8, 1.0, b_group=2)
    with pytest.raises(ValueError):
        ops.bmm_i8_softmax_q8(a, b, 1.0, b_group=4)
    with pytest.raises(ValueError, match="multiple"):                                         # the raw entry's own check
        L.check(L.lib().asq_bmm_i8(a.data_ptr(), b.data_ptr(), a.data_ptr(), 2 | L.ASQ_BMM_B_GROUP(3), 4, 8, 16, 32, 1.0, None))


# (lead, Hq, Hkv, Sq, Sk, d, causal) -> the route: (b_group, M of the two products, causal flag of the call)
ATT = [(((2,), 8, 2, 160, 160, 64, True), (4, 160, True)),       # grouped
       (((2,), 8, 2, 70, 200, 96, False), (1, 280, False)),      # fold
       (((3,), 8, 2, 1, 300, 128, True), (1, 4, False))]         # decode fold: the causal flag is dropped


@pytest.mark.parametrize("case", ATT, ids=["causal-grouped", "full-fold", "decode-fold"])
def test_int8_attention_gqa_equals_mha_on_expanded_kv(case, monkeypatch):
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    (lead, hq, hkv, sq, sk, d, causal), (group, m, flag) = case
    r = hq // hkv
    calls = []
    real_sm, real_kn = ops.bmm_i8_softmax_q8, ops.bmm_i8_kn

    def spy_sm(a, b, *args, **kw):
        calls.append(("softmax", tuple(a.shape), b.data_ptr(), kw.get("b_group", 1), args[1] if len(args) > 1 else kw.get("causal", False)))
        return real_sm(a, b, *args, **kw)

    def spy_kn(a, b, *args, **kw):
        calls.append(("kn", tuple(a.shape), b.data_ptr(), kw.get("b_group", 1), None))
        return real_kn(a, b, *args, **kw)

    monkeypatch.setattr(ops, "bmm_i8_softmax_q8", spy_sm)
    monkeypatch.setattr(ops, "bmm_i8_kn", spy_kn)
    g = torch.Generator().manual_seed(77)
    q = torch.randint(-128, 128, (*lead, hq, sq, d), generator=g, dtype=torch.int8).to(DEV)
    k = torch.randint(-128, 128, (*lead, hkv, sk, d), generator=g, dtype=torch.int8).to(DEV)
    v = torch.randint(-128, 128, (*lead, hkv, sk, d), generator=g, dtype=torch.int8).to(DEV)
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=d ** -0.5 * 20, causal=causal).cuda()
    out = att(q, k, v)
    torch.cuda.synchronize()
    nb = lead[0] * hq if group > 1 else lead[0] * hkv
    assert calls == [("softmax", (nb, m, d), k.data_ptr(), group, flag), ("kn", (nb, m, sk), v.data_ptr(), group, None)], calls
    del calls[:]
    want = att(q, k.repeat_interleave(r, -3), v.repeat_interleave(r, -3))
    assert [c[3] for c in calls] == [1, 1] and calls[0][1] == (lead[0] * hq, sq, d)             # the MHA route is today's
    assert out.shape == q.shape and out.dtype == torch.int8 and out.is_contiguous() and torch.equal(out, want)
    assert int(out.abs().max()) > 20                                                           # the scales leave a signal


def test_int8_attention_gqa_shape_errors():
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    att = Int8Attention.from_scale(0.1, 0.1, 0.1, 0.1).cuda()
    z = lambda *shape: torch.zeros(shape, dtype=torch.int8, device=DEV)
    for qs, ks in (((2, 6, 5, 16), (2, 4, 7, 16)), ((3, 8, 5, 16), (2, 2, 7, 16)), ((8, 5, 16), (2, 2, 7, 16)), ((2, 2, 5, 16), (2, 8, 7, 16))):
        with pytest.raises(ValueError, match="shape mismatch"):
            att(z(*qs), z(*ks), z(*ks))
    assert att(z(8, 5, 16), z(2, 7, 16), z(2, 7, 16)).shape == (8, 5, 16)                      # 3-D: the head dim is the only leading dim


def test_decode_gqa_is_faster_than_expanding_kv():
    """A decode step of 16 sequences, 32 query heads over 8 KV heads, d = 128, 4096 cached keys: the grouped-query forward against the only route there was,
    repeat_interleave of k and v followed by the multi-head forward -- the same products on 4x the K / V bytes plus two copies, so no margin is added.
    HIP events, the two alternating call by call, median of 20 after 5 warm-ups, 3 operand sets in rotation (the expanded K + V alone is 512 MiB per
    set, beyond the 256 MiB Infinity Cache)."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, hq, hkv, sk, d, nrot = 16, 32, 8, 4096, 128, 3
    r = hq // hkv
    torch.manual_seed(47)
    Q = [torch.randint(-128, 128, (B, hq, 1, d), dtype=torch.int8, device=DEV) for _ in range(nrot)]
    Kc = [torch.randint(-128, 128, (B, hkv, sk, d), dtype=torch.int8, device=DEV) for _ in range(nrot)]
    Vc = [torch.randint(-128, 128, (B, hkv, sk, d), dtype=torch.int8, device=DEV) for _ in range(nrot)]
    assert 2 * r * Kc[0].numel() > 256 << 20
    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=d ** -0.5 * 20, causal=True).cuda()
    gqa = lambda i: att(Q[i], Kc[i], Vc[i])
    expand = lambda i: att(Q[i], Kc[i].repeat_interleave(r, 1), Vc[i].repeat_interleave(r, 1))
    assert torch.equal(gqa(0), expand(0))
    t_gqa, t_expand = medians_us((gqa, expand), nrot)
    print(f"decode 16 x 32/8 heads x 4096 keys: GQA forward {t_gqa:.1f} us, repeat_interleave + MHA forward {t_expand:.1f} us")
    del Q, Kc, Vc
    torch.cuda.empty_cache()
    assert t_gqa < t_expand, f"GQA forward {t_gqa:.1f} us, repeat_interleave + MHA forward {t_expand:.1f} us"
