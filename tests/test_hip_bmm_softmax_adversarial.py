"""GPU: bmm_i8_sm128 (asq_bmm_i8 with ASQ_BMM_S8 | ASQ_BMM_SOFTMAX [| ASQ_BMM_CAUSAL]) on ordered scores -- tests/softmax_q8_adversarial.py's operands through
ops.bmm_i8_softmax_q8, the raw C entry and Int8Attention.forward.

The hard staircase, its ties and the score-range cases are compared byte for byte with bytes known by design (one-hot rows: no band, no reference arithmetic).
Every other case is judged by softmax_q8_ref.check: the float64 target, the derived tie band, BAND_CAP.  tests/test_softmax_adversarial_cpu.py re-derives the band
share of every case here from the same seeds and asserts which arithmetic fault each family rejects.  Full and causal, batch 1 and 3 (the entries hold different
bytes, shuffles and query signs), and the staircase and one soft ramp through all twelve instantiations <CAUSAL, FAST, GROUPED, TOKEN>."""
import numpy as np
import pytest
import torch

import softmax_q8_adversarial as A
import softmax_q8_ref as R
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from bmm_ref import ref_out

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SM = L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX


def dev(x):
    return torch.from_numpy(np.array(x, order="C")).to(DEV)             # a copy: the shared operands are read-only


def fused(a, b, alpha, causal, **kw):
    out = ops.bmm_i8_softmax_q8(a if torch.is_tensor(a) else dev(a), b if torch.is_tensor(b) else dev(b), alpha, causal, **kw)
    torch.cuda.synchronize()
    assert out.dtype == torch.int8 and out.is_contiguous()
    return out.cpu().numpy()


def token(x):
    """[S, heads, rows, cols] -> [S, rows, heads, cols]"""
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3))


def raw_offset_call(a, b, flags, batch, M, N, K, alpha, oa, ob, oo):
    """asq_bmm_i8 on copies of a and b that start oa / ob bytes behind a 16-B aligned address, into a buffer pre-filled with 0x5A at byte offset oo: -> the [batch, M, N]
    result, after checking that nothing around it was written"""
    abuf = torch.zeros(a.size + 16, dtype=torch.int8, device=DEV)
    bbuf = torch.zeros(b.size + 16, dtype=torch.int8, device=DEV)
    obuf = torch.full((batch * M * N + 32,), 0x5A, dtype=torch.int8, device=DEV)
    a_t, b_t, o_t = abuf[oa:oa + a.size], bbuf[ob:ob + b.size], obuf[oo:oo + batch * M * N]
    a_t.copy_(dev(a).flatten()), b_t.copy_(dev(b).flatten())
    assert a_t.data_ptr() % 16 == oa and b_t.data_ptr() % 16 == ob and o_t.data_ptr() % 16 == oo
    L.check(L.lib().asq_bmm_i8(a_t.data_ptr(), b_t.data_ptr(), o_t.data_ptr(), flags, batch, M, N, K, alpha, torch.cuda.current_stream().cuda_stream), "asq_bmm_i8")
    torch.cuda.synchronize()
    assert torch.all(obuf[:oo] == 0x5A) and torch.all(obuf[oo + batch * M * N:] == 0x5A), "bytes around the result were written"
    return o_t.view(batch, M, N).cpu().numpy()


# ---- families b and e: by design, byte for byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.HARD_CASES, ids=A.case_id)
def test_hard_staircase_is_one_hot(case):
    """neighbouring keys >= 100 nats apart (alpha 1 and 1e3: up to 1e9): 127 on the best visible key -- n = m + N - M for a +127 query under the mask, N - 1 without
    it, 0 for a -127 query, the other end for a negative alpha -- rne(127 / g) on g equal leaders, 0 elsewhere and on rows without a key"""
    shape, tie, alpha = case
    M, N, K = shape
    alpha = A.hard_alpha(K) if alpha is None else alpha
    for batch in A.BATCHES:
        a, b, levels, signs = A.hard_operands(shape, batch, tie)
        a_t, b_t = dev(a), dev(b)
        for causal in (False, True):
            assert ops.bmm_kernel_name(batch, M, N, K, SM | (L.ASQ_BMM_CAUSAL if causal else 0)) == "sm128"
            want, half = A.hard_want(shape, levels, signs, causal, alpha < 0)
            q = fused(a_t, b_t, alpha, causal)
            A.check_one_hot(q, want, half, f"{A.case_id(case)} batch={batch} causal={causal}")


# ---- families c, d and the 2^24 case of e: the band rule --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.BAND_CASES, ids=A.case_id)
def test_ordered_scores_by_the_band_rule(case):
    for batch in A.BATCHES:
        a, b, alpha = A.band_operands(case, batch)
        M, N = a.shape[1], b.shape[1]
        a_t, b_t = dev(a), dev(b)
        acc = R.acc_exact(a, b)
        if case[0] == "big":
            assert acc.max() > 2 ** 24
        for causal in (False, True):
            q = fused(a_t, b_t, alpha, causal)
            assert q.shape == acc.shape and q.min() >= 0
            t = R.target(acc, alpha, causal)
            what = f"{A.case_id(case)} batch={batch} causal={causal}"
            nband, ndiff = R.check(q, t, N, what)
            print(f"{what}: in band {nband}, q != rne(t) {ndiff} of {t.size}")
            assert np.all(q[:, ~R.visible(M, N, causal)] == 0)
        if case[0] == "soft" and case[3] != "asc":
            # one multiset of scores per row in every order: outside the band the bytes, un-permuted, are the ascending order's bytes (full rows: every row sees every key)
            _, shape, nats, order = case
            src = A.soft_operands(shape, batch, order)[2]
            a0, b0, _ = A.soft_operands(shape, batch, "asc")
            assert np.array_equal(a0, a) and all(np.array_equal(b[i], b0[i][src[i]]) for i in range(batch))
            q, q0 = fused(a_t, b_t, alpha, False), fused(a0, b0, alpha, False)
            t0 = R.target(R.acc_exact(a0, b0), alpha, False)
            for i in range(batch):
                clear = ~(R.in_band(t0[i], N)[:, src[i]] | R.in_band(R.target(acc[i:i + 1], alpha, False)[0], N))
                assert np.array_equal(q[i][clear], q0[i][:, src[i]][clear]), f"{A.case_id(case)} entry {i}: differs from the ascending order"


# ---- family e: alphas of no effect ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_alphas_of_no_effect_give_the_uniform_rows(causal):
    """alpha = 1e-30, a denormal, -0.0, 0.0 on random operands: the bytes of the zero-a call (every visible key 1 / n_vis), whatever the operands hold"""
    for shape in ((2, 40, 24, 64), (2, 130, 300, 32), (3, 150, 141, 33)):
        B, M, N, K = shape
        a, b = R.operands((M, N, K), B)
        a_t, b_t = dev(a), dev(b)
        uniform = fused(np.zeros_like(a), b_t, 0.37, causal)
        vis = R.visible(M, N, causal)
        t = np.broadcast_to(np.where(vis, 127.0 / np.maximum(vis.sum(1), 1)[:, None], 0.0)[None], uniform.shape)
        band = R.in_band(t, N)
        assert np.array_equal(uniform[~band], np.rint(t[~band]).astype(np.int8))
        for alpha in A.NULL_ALPHAS:
            assert np.array_equal(fused(a_t, b_t, alpha, causal), uniform), f"{shape} alpha={alpha!r}"


# ---- all twelve instantiations <CAUSAL, FAST, GROUPED, TOKEN> ------------------------------------------------------------------------------------------------
def form_calls(form, a, b, S, h, r, alpha, causal, path):
    """the result of the form's own call on head-major a [S * h, M, K] and b [S * h / r, N, K].  path "skew": through the C entry on operands one byte (a) and three
    bytes (b) off alignment, which takes the byte path at K % 16 == 0; otherwise through ops.bmm_i8_softmax_q8"""
    M, N, K = a.shape[1], b.shape[1], a.shape[2]
    flags = SM | (L.ASQ_BMM_CAUSAL if causal else 0)
    if form.startswith("token"):
        ta, tb = token(a.reshape(S, h, M, K)), token(b.reshape(S, h // r, N, K))
        if path != "skew":
            return fused(ta, tb, alpha, causal, b_group=r)
        flags |= L.ASQ_BMM_A_TOKEN | L.ASQ_BMM_B_TOKEN | L.ASQ_BMM_HEADS(h) | (L.ASQ_BMM_B_GROUP(r) if r > 1 else 0)
        return raw_offset_call(ta, tb, flags, S * h, M, N, K, alpha, 1, 3, 1)
    if path != "skew":
        return fused(a, b, alpha, causal, b_group=r)
    return raw_offset_call(a, b, flags | (L.ASQ_BMM_B_GROUP(r) if r > 1 else 0), S * h, M, N, K, alpha, 1, 3, 1)


@pytest.mark.parametrize("path", ["k64", "k33", "skew"])
@pytest.mark.parametrize("form", list(A.FORMS))
def test_every_instantiation_on_the_staircase_and_a_soft_ramp(form, path):
    """plain / GROUPED (r = 4, 8: the r query heads of a group differ in sign) / TOKEN (token-major a and b, another staircase per head and sequence, without and
    with a group) x FAST (K = 64, aligned) / the byte path (K = 33; K = 64 one byte off) x full / causal.  Each result against the by-design bytes (staircase) or
    the band rule (soft ramp), and bit for bit against the plain dense call on expanded, head-major, aligned copies."""
    S, h, r = A.FORMS[form]
    shape = M, N, K = A.FORM_SHAPES["k33" if path == "k33" else "k64"]
    for ties, alpha in ((True, A.hard_alpha(K)), (False, A.soft_alpha(N, K, 0.45))):
        a, b, levels, signs = A.head_operands(shape, S, h, r, ties)
        b_all = b[np.arange(S * h) // r]
        acc = R.acc_exact(a, b_all)
        for causal in (False, True):
            what = f"{form} {path} {'staircase' if ties else 'soft ramp'} causal={causal}"
            got = form_calls(form, a, b, S, h, r, alpha, causal, path)
            assert got.shape == (S * h, M, N)
            if ties:
                want, half = A.head_want(shape, levels, signs, r, causal)
                A.check_one_hot(got, want, half, what)
            else:
                R.check(got, R.target(acc, alpha, causal), N, what)
            if form != "plain" or path == "skew":
                assert np.array_equal(got, fused(a, b_all, alpha, causal)), f"{what}: differs from the plain call on expanded head-major copies"


# ---- Int8Attention.forward on the staircase ------------------------------------------------------------------------------------------------------------------
# (layout, B, Hq, Hkv, Sq, Sk, d, causal)
ATT = [("bhsd", 2, 2, 2, 140, 300, 64, True), ("bshd", 2, 3, 3, 140, 300, 64, True), ("bhsd", 1, 8, 2, 140, 300, 64, True), ("bshd", 2, 4, 2, 300, 140, 144, True),
       ("bhsd", 1, 4, 2, 70, 300, 128, False), ("bshd", 1, 4, 4, 130, 257, 33, False)]


@pytest.mark.parametrize("case", ATT, ids=lambda c: "-".join(map(str, c)))
def test_int8_attention_returns_the_row_of_v_the_staircase_points_at(case):
    """P is one-hot by design, so row m of the output is epilogue(127 * V[the row's best visible key]) exactly -- V[m + Sk - Sq] for a +127 query under the mask -- and
    0 for a row without a key; V[n, :] is a pattern of its own per key and head, so a neighbouring key gives other bytes"""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    layout, B, hq, hkv, sq, sk, d, causal = case
    r = hq // hkv
    shape = (sq, sk, d)
    a, b, levels, signs = A.head_operands(shape, B, hq, r, False)
    v = ((37 * np.arange(sk)[None, :, None] + 11 * np.arange(d)[None, None, :] + 5 * np.arange(B * hkv)[:, None, None]) % 255 - 127).astype(np.int8)
    att = Int8Attention.from_scale(A.hard_alpha(d), 1.0, 1.0, 1.0, causal=causal).cuda()
    assert att.qk_bmm.a.item() == np.float32(A.hard_alpha(d))
    q4, k4, v4 = a.reshape(B, hq, sq, d), b.reshape(B, hkv, sk, d), v.reshape(B, hkv, sk, d)
    if layout == "bshd":
        out = att(dev(token(q4)), dev(token(k4)), dev(token(v4)), layout="bshd")
        torch.cuda.synchronize()
        assert tuple(out.shape) == (B, sq, hq, d)
        out = out.permute(0, 2, 1, 3)
    else:
        out = att(dev(q4), dev(k4), dev(v4))
        torch.cuda.synchronize()
        assert tuple(out.shape) == (B, hq, sq, d)
    out = out.cpu().numpy().reshape(B * hq, sq, d)
    want_p, half = A.head_want(shape, levels, signs, r, causal)
    assert not half.any() and set(np.unique(want_p)) <= {0, 127}
    v_all = v[np.arange(B * hq) // r].astype(np.int64)
    want = ref_out(np.einsum("emn,end->emd", want_p.astype(np.int64), v_all), torch.int8, att.pv_bmm.a.item())
    assert np.array_equal(out, want), f"{case}: {(out != want).any(-1).sum()} rows differ"
    m = np.flatnonzero(R.visible(sq, sk, causal).any(1))
    own = m + sk - sq if causal else np.full(len(m), sk - 1)
    assert (signs[0] == 1).all() and np.array_equal(out[0][m], ref_out(127 * v_all[0][own], torch.int8, att.pv_bmm.a.item()))
    assert not out[:, ~R.visible(sq, sk, causal).any(1)].any() and np.abs(out).max() > 100
