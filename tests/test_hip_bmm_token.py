"""GPU: the batched int8 matmuls on token-major operands (ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN with ASQ_BMM_HEADS(h) on asq_bmm_i8's out_kind; a 4-D a or
b, `out_token=True` and `heads=` on ops.bmm_i8 / bmm_i8_kn / bmm_i8_softmax_q8) and Int8Attention's layout="bshd" on top of them.

A flagged call is the same kernel form with other addresses, so the first yardstick is the same op on head-major contiguous copies
(.permute(0, 2, 1, 3).contiguous()) of the flagged operands, bit for bit, the token-major result permuted back.  The second does not rest on the library:
the int32 kinds against an int64 einsum in numpy, the softmax kinds against softmax_q8_ref's target by its own band rule.

The shapes are the smallest that reach each form's edges: M in {1, 5, 16} (m16 / m16kn) and {17, 130} (t128 / t128kn / sm128), N in {1, 70, 129, 257}
(and 64 / 128 for the 16-B load path of a row-major b and the vector stores), K in {16, 48, 128} (16-B loads) and {5, 33} (byte path), h in {2, 3, 4, 128},
r in {1, 2, 4}, 1 or 3 sequences; 2 x 4 x 130 x 257 x 128 walks several tiles per entry and the XCD remap."""
import numpy as np
import pytest
import torch

import softmax_q8_ref as R
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, ref_out, tbits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KINDS = (torch.int32, torch.float32, torch.int8)
ALPHA = 0.0123

# (sequences, h, r, M, N, K, kn, flagged operands): every non-empty subset of a / b / o on both layouts of b, every kind in each case
PLAIN = [(1, 2, 1, 1, 1, 16, False, "a"), (3, 3, 1, 5, 70, 5, False, "b"), (1, 2, 2, 16, 129, 48, False, "o"), (3, 4, 2, 17, 70, 33, False, "ab"),
         (1, 3, 1, 130, 129, 16, False, "ao"), (3, 2, 1, 17, 257, 128, False, "bo"), (2, 4, 4, 130, 257, 128, False, "abo"),
         (1, 128, 4, 5, 70, 16, False, "abo"), (3, 2, 2, 16, 64, 128, False, "abo"),
         (3, 3, 1, 1, 70, 33, True, "a"), (1, 2, 2, 5, 1, 48, True, "b"), (3, 4, 4, 16, 257, 128, True, "o"), (1, 4, 2, 17, 129, 5, True, "ab"),
         (3, 2, 1, 130, 70, 16, True, "ao"), (1, 128, 2, 17, 129, 48, True, "bo"), (2, 4, 2, 130, 257, 128, True, "abo"),
         (3, 4, 2, 5, 128, 48, True, "abo"), (1, 2, 1, 130, 128, 128, True, "abo")]
# (sequences, h, r, M, N, K, flagged operands): out stays dense
SOFTMAX = [(3, 3, 1, 5, 70, 5, "a"), (1, 2, 2, 17, 129, 48, "b"), (2, 4, 2, 130, 257, 128, "ab"), (1, 4, 4, 16, 70, 33, "ab"), (3, 2, 1, 130, 1, 16, "a"),
           (1, 128, 2, 1, 70, 16, "ab"), (1, 2, 1, 130, 70, 16, "ab")]          # the last: causal rows without a visible key


def ident(case):
    return "x".join(str(int(c)) if isinstance(c, bool) else str(c) for c in case)


def dev(x, skew=0):
    """x on the device, contiguous; skew: its first byte that many bytes behind a 256-B aligned address"""
    x = np.ascontiguousarray(x)
    if not skew:
        return torch.from_numpy(x).to(DEV)
    flat = torch.empty((x.size + skew,), dtype=torch.int8, device=DEV)
    t = flat[skew:].view(*x.shape)
    t.copy_(torch.from_numpy(x))
    assert t.is_contiguous() and t.data_ptr() % 16 == skew
    return t


def operands(S, h, r, M, N, K, kn):
    """head-major numpy operands: a [S, h, M, K], b [S, h / r, N, K] or (kn) [S, h / r, K, N]"""
    rng = np.random.default_rng(5100 + 1000 * S + 100 * h + 10 * r + M + 7 * N + 13 * K + kn)
    return rng.integers(-128, 128, (S, h, M, K), dtype=np.int8), rng.integers(-128, 128, (S, h // r, K, N) if kn else (S, h // r, N, K), dtype=np.int8)


def token(x):
    """[S, heads, rows, cols] -> [S, rows, heads, cols]"""
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3))


def dense(x):
    return x.reshape(-1, *x.shape[2:])


def head_major(t):
    """a token-major device tensor [S, rows, heads, cols] as the dense [S * heads, rows, cols] copy"""
    t = t.permute(0, 2, 1, 3).contiguous()
    return t.view(-1, *t.shape[2:])


def acc_exact(a, b, r, kn):
    """[S * h, M, N] int64 from the head-major operands: head x of a sequence meets b head x // r"""
    bb = b.astype(np.int64)[:, np.arange(a.shape[1]) // r]
    return dense(np.einsum("shmk,shkn->shmn" if kn else "shmk,shnk->shmn", a.astype(np.int64), bb))


def softmax_alpha(K):
    """a score standard deviation of about 4 (softmax_q8_ref.alphas)"""
    return float(np.float32(4.0 / (5461.0 * np.sqrt(max(K, 1)))))


def args_of(a, b, flagged, h, skew=0):
    """the operands of a flagged call (token-major where flagged, dense otherwise) and its keywords"""
    ta = dev(token(a) if "a" in flagged else dense(a), skew)
    tb = dev(token(b) if "b" in flagged else dense(b), skew)
    return ta, tb, {"heads": h} if "a" not in flagged else {}


@pytest.mark.parametrize("case", PLAIN, ids=ident)
def test_flagged_call_is_the_base_kind_on_head_major_copies(case):
    S, h, r, M, N, K, kn, flagged = case
    a, b = operands(S, h, r, M, N, K, kn)
    op = ops.bmm_i8_kn if kn else ops.bmm_i8
    ta, tb, kw = args_of(a, b, flagged, h)
    da = head_major(ta) if "a" in flagged else ta
    db = head_major(tb) if "b" in flagged else tb
    flags = sum(f for c, f in (("a", L.ASQ_BMM_A_TOKEN), ("b", L.ASQ_BMM_B_TOKEN), ("o", L.ASQ_BMM_OUT_TOKEN)) if c in flagged)
    acc = acc_exact(a, b, r, kn)
    assert np.abs(acc).max() < 2 ** 31
    for kind in KINDS:
        got = op(ta, tb, kind, ALPHA, b_group=r, out_token="o" in flagged, **kw)
        want = op(da, db, kind, ALPHA, b_group=r)
        assert got.dtype == kind and got.is_contiguous() and tuple(got.shape) == ((S, M, h, N) if "o" in flagged else (S * h, M, N))
        if "o" in flagged:
            got = head_major(got)
        assert torch.equal(tbits(got), tbits(want)), f"{kind} {case}: differs from the call on head-major copies"
        assert_bits_equal(got.cpu().numpy(), ref_out(acc.astype(np.int32), kind, ALPHA), f"{kind} {case}")
        code = ops._BMM_KIND[kind] | (L.ASQ_BMM_B_KN if kn else 0) | L.ASQ_BMM_B_GROUP(r)
        name = ops.bmm_kernel_name(S * h, M, N, K, code | flags | L.ASQ_BMM_HEADS(h))
        assert name == ops.bmm_kernel_name(S * h, M, N, K, code) == ("m16" if M <= 16 else "t128") + ("kn" if kn else "")


@pytest.mark.parametrize("case", [(3, 3, 1, 17, 70, 48, False, "abo"), (3, 4, 2, 5, 128, 48, True, "abo"), (1, 2, 2, 130, 70, 16, True, "ab")], ids=ident)
def test_operands_offset_by_one_byte(case):
    S, h, r, M, N, K, kn, flagged = case
    a, b = operands(S, h, r, M, N, K, kn)
    op = ops.bmm_i8_kn if kn else ops.bmm_i8
    ta, tb, kw = args_of(a, b, flagged, h, skew=1)
    acc = acc_exact(a, b, r, kn).astype(np.int32)
    for kind in KINDS:
        got = op(ta, tb, kind, ALPHA, b_group=r, out_token="o" in flagged, **kw)
        want = op(head_major(ta), head_major(tb), kind, ALPHA, b_group=r)
        got = head_major(got) if "o" in flagged else got
        assert torch.equal(tbits(got), tbits(want)), f"{kind} {case}"
        assert_bits_equal(got.cpu().numpy(), ref_out(acc, kind, ALPHA), f"{kind} {case}")
    if not kn:
        for causal in (False, True):
            assert torch.equal(ops.bmm_i8_softmax_q8(ta, tb, softmax_alpha(K), causal, b_group=r),
                               ops.bmm_i8_softmax_q8(head_major(ta), head_major(tb), softmax_alpha(K), causal, b_group=r))


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("case", SOFTMAX, ids=ident)
def test_flagged_softmax_is_the_base_kind_on_head_major_copies(case, causal):
    S, h, r, M, N, K, flagged = case
    a, b = operands(S, h, r, M, N, K, False)
    ta, tb, kw = args_of(a, b, flagged, h)
    alpha = softmax_alpha(K)
    got = ops.bmm_i8_softmax_q8(ta, tb, alpha, causal, b_group=r, **kw)
    want = ops.bmm_i8_softmax_q8(head_major(ta) if "a" in flagged else ta, head_major(tb) if "b" in flagged else tb, alpha, causal, b_group=r)
    assert got.dtype == torch.int8 and tuple(got.shape) == (S * h, M, N) and got.is_contiguous()
    assert torch.equal(got, want), f"{case} causal={causal}: differs from the call on head-major copies"
    assert int(want.max()) > 0
    flags = sum(f for c, f in (("a", L.ASQ_BMM_A_TOKEN), ("b", L.ASQ_BMM_B_TOKEN)) if c in flagged)
    code = 18 | (L.ASQ_BMM_CAUSAL if causal else 0) | L.ASQ_BMM_B_GROUP(r)
    assert ops.bmm_kernel_name(S * h, M, N, K, code | flags | L.ASQ_BMM_HEADS(h)) == "sm128"
    if causal and M > N:
        assert not got[:, :M - N].any() and got[:, M - N].any()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_softmax_kinds_against_numpy(causal):
    """softmax_q8_ref's own operands of 130 x 70 x 200 at batch 32, read as 4 sequences of 8 heads"""
    M, N, K = shape = (130, 70, 200)
    a, b = R.operands(shape, 32)
    alpha = R.alphas(shape)[1]
    ta, tb = dev(token(a.reshape(4, 8, M, K))), dev(token(b.reshape(4, 8, N, K)))
    got = ops.bmm_i8_softmax_q8(ta, tb, alpha, causal).cpu().numpy()
    assert got.min() >= 0
    R.check(got, R.target(R.acc_exact(a, b), alpha, causal), N, f"{shape} causal={causal}")


def test_a_sequences_bytes_do_not_depend_on_the_other_sequences():
    S, h, r, M, N, K = 3, 4, 2, 20, 70, 48
    for kn in (False, True):
        a, b = operands(S, h, r, M, N, K, kn)
        op = ops.bmm_i8_kn if kn else ops.bmm_i8
        ta, tb = dev(token(a)), dev(token(b))
        for kind in KINDS:
            many = op(ta, tb, kind, ALPHA, b_group=r, out_token=True)
            assert torch.equal(tbits(many), tbits(op(ta, tb, kind, ALPHA, b_group=r, out_token=True)))          # deterministic
            for s in range(S):
                one = op(ta[s:s + 1], tb[s:s + 1], kind, ALPHA, b_group=r, out_token=True)
                assert torch.equal(tbits(many[s:s + 1]), tbits(one)), (kn, kind, s)


def test_bad_token_arguments_raise_before_launch():
    z = lambda *shape: torch.zeros(shape, dtype=torch.int8, device=DEV)
    a4, a3, b4, b3 = z(2, 5, 4, 16), z(8, 5, 16), z(2, 7, 4, 16), z(8, 7, 16)
    for call in (lambda: ops.bmm_i8(a4, z(2, 7, 3, 16), torch.int8),                       # b's heads
                 lambda: ops.bmm_i8(a4, z(3, 7, 4, 16), torch.int8),                       # b's sequences
                 lambda: ops.bmm_i8(a4, z(2, 7, 4, 32), torch.int8),                       # K
                 lambda: ops.bmm_i8(a4, b4, torch.int8, b_group=2),                        # b must then hold 2 heads
                 lambda: ops.bmm_i8(a4, z(2, 7, 1, 16), torch.int8, b_group=3),            # 4 heads, groups of 3
                 lambda: ops.bmm_i8(a4, b3, torch.int8, heads=2),                          # heads disagrees with a
                 lambda: ops.bmm_i8(a3, b4, torch.int8),                                   # heads missing
                 lambda: ops.bmm_i8(a3, b3, torch.int8, out_token=True),
                 lambda: ops.bmm_i8(a3, b3, torch.int8, out_token=True, heads=3),          # 8 entries, 3 heads
                 lambda: ops.bmm_i8(a3, b3, torch.int8, heads=4),                          # heads without a token-major operand
                 lambda: ops.bmm_i8(z(2, 5, 1, 16), z(2, 7, 1, 16), torch.int8),           # one head is the dense layout
                 lambda: ops.bmm_i8(z(1, 5, 129, 16), z(1, 7, 129, 16), torch.int8),       # more heads than the field holds
                 lambda: ops.bmm_i8(a4.transpose(1, 2), b4, torch.int8),                   # not contiguous
                 lambda: ops.bmm_i8_kn(a4, b4, torch.int8),                                # [S, K, H, N] wanted
                 lambda: ops.bmm_i8(z(2, 2, 5, 4, 16), b4, torch.int8)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(TypeError):
        ops.bmm_i8_softmax_q8(a4, b4, 0.1, out_token=True)                                  # P stays dense: the op has no such argument
    with pytest.raises(ValueError, match="heads"):                                          # the raw entry's own check
        L.check(L.lib().asq_bmm_i8(a3.data_ptr(), b3.data_ptr(), a3.data_ptr(), 2 | L.ASQ_BMM_A_TOKEN | L.ASQ_BMM_HEADS(3), 8, 5, 7, 16, 1.0, None))


# (B, Sq, Sk, Hq, Hkv, d, causal) -> the two calls: (a's shape, b's dims, b_group, heads keyword, causal flag, out_token)
ATT = [((2, 140, 140, 4, 4, 64, False), ((2, 140, 4, 64), 4, 1, None, False, True)),            # MHA prefill
       ((2, 150, 150, 8, 2, 64, True), ((2, 150, 8, 64), 4, 4, None, True, True)),              # GQA causal prefill: the heads share b
       ((3, 1, 300, 8, 2, 128, True), ((6, 4, 128), 4, 1, 2, False, False)),                    # GQA decode: the group is a's rows, the causal flag is dropped
       ((1, 1, 200, 8, 2, 128, True), ((2, 4, 128), 4, 1, 2, False, False))]                    # one sequence on a prefix of a larger cache


@pytest.mark.parametrize("case", ATT, ids=["mha-prefill", "gqa-causal-prefill", "gqa-decode-fold", "cache-prefix"])
def test_int8_attention_bshd_equals_bhsd_on_permuted_copies(case, monkeypatch):
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    (B, sq, sk, hq, hkv, d, causal), (a_shape, b_dim, group, heads, flag, out_token) = case
    g = torch.Generator().manual_seed(91)
    q = torch.randint(-128, 128, (B, sq, hq, d), generator=g, dtype=torch.int8).to(DEV)
    smax = sk + 56 if B == 1 else sk
    kc = torch.randint(-128, 128, (B, smax, hkv, d), generator=g, dtype=torch.int8).to(DEV)
    vc = torch.randint(-128, 128, (B, smax, hkv, d), generator=g, dtype=torch.int8).to(DEV)
    k, v = kc[:, :sk], vc[:, :sk]                                                              # with B == 1: a view of the cache, no copy
    assert k.data_ptr() == kc.data_ptr() and v.data_ptr() == vc.data_ptr()
    calls = []
    real_sm, real_kn = ops.bmm_i8_softmax_q8, ops.bmm_i8_kn

    def spy_sm(a, b, alpha, causal=False, **kw):
        calls.append(("softmax", tuple(a.shape), a.data_ptr(), b.dim(), b.data_ptr(), kw.get("b_group", 1), kw.get("heads"), causal, False))
        return real_sm(a, b, alpha, causal, **kw)

    def spy_kn(a, b, *args, **kw):
        calls.append(("kn", tuple(a.shape), None, b.dim(), b.data_ptr(), kw.get("b_group", 1), kw.get("heads"), None, kw.get("out_token", False)))
        return real_kn(a, b, *args, **kw)

    att = Int8Attention.from_scale(0.011, 0.013, 0.02, 0.004, sm_scale=d ** -0.5 * 20, causal=causal).cuda()
    want = att(q.permute(0, 2, 1, 3).contiguous(), k.permute(0, 2, 1, 3).contiguous(), v.permute(0, 2, 1, 3).contiguous()).permute(0, 2, 1, 3)
    monkeypatch.setattr(ops, "bmm_i8_softmax_q8", spy_sm)
    monkeypatch.setattr(ops, "bmm_i8_kn", spy_kn)
    out = att(q, k, v, layout="bshd")
    torch.cuda.synchronize()
    m = a_shape[1]
    p_shape = (B * hq, sq, sk) if out_token else (a_shape[0], m, sk)
    assert calls == [("softmax", a_shape, q.data_ptr(), b_dim, k.data_ptr(), group, heads, flag, False),
                     ("kn", p_shape, None, b_dim, v.data_ptr(), group, hq if out_token else heads, None, out_token)], calls     # two launches, no operand copied
    assert tuple(out.shape) == (B, sq, hq, d) and out.dtype == torch.int8 and out.is_contiguous()
    assert torch.equal(out, want), "differs from the head-major forward on permuted copies"
    assert int(out.abs().max()) > 20                                                           # the scales leave a signal
