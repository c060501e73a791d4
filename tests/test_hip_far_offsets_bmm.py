"""GPU: the batched int8 matmuls (csrc/asq_bmm.hip: bmm_i8, bmm_i8_kn, bmm_i8_softmax_q8) on operands and outputs beyond 2^32 bytes (tests/far_offsets.py states the
rule: whole equals parts, bit for bit, on the device).

  * far a: 4100 x 1024 x 1024 (4.3 GB) against a small N = 32, dense and with b_group = 2;
  * far b: the same bytes as [B, N, K] for bmm_i8 / bmm_i8_softmax_q8 and as [B, K, N] for bmm_i8_kn, against a small M = 32 and M = 16 (the narrow kernels);
  * far out: 4100 x 1024 x 1024 int8 at K = 16 -- EVERY batch is compared (test_hip_bmm.py's test beyond 2^31 elements checks five) -- and 1030 batches of fp32 / int32;
  * token-major: a [S = 1030, 1024, h = 4, 1024] with out_token, so that the magic-number head division runs at large entry indices; b token-major too, and grouped; bmm_i8, bmm_i8_kn and the softmax form.

Each whole call is compared with the same call on batch chunks (sequence chunks for the token-major forms).  a far operand sits 2^31 bytes into an arena of 0x55 and
is unchanged afterwards.  The CPU anchor: the batches on each side of byte offsets 2^31 and 2^32, the first and the last, through a NumPy integer matmul and
tests/bmm_ref.py::ref_out; the softmax form's anchor is the whole-equals-chunks rule alone (its yardstick, tests/attn_decode_ref.py's interval, is per row of a chunk)."""
import numpy as np
import pytest
import torch

import far_offsets as F
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, ref_out, tbits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B_FAR, B_F32, SIDE, SMALL, STEP = F.BMM_B, F.BMM_B32, 1024, 32, 256
ALPHA = 1.0 / 700


def _i8(shape, seed):
    return torch.randint(-128, 128, shape, dtype=torch.int8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _far(shape, seed):
    n = int(np.prod(shape))
    ar = F.Arena(n, DEV)
    ar.fill_random(0, n, seed)
    pitch = n // shape[0]
    idx = F.anchor_rows(pitch, shape[0], 2)
    for i in idx:
        if i * pitch >= F.G31:
            ar.differs_below(i * pitch, 4096)
    return ar, ar.view(torch.int8, shape), idx


def _batches_equal(what, whole, part, n, step):
    for a, b in F.chunks(n, step):
        assert torch.equal(tbits(whole[a:b]), tbits(part(a, b))), f"{what}: entries {a} .. {b} of the whole call differ from the chunk's own call"


def _acc(a, b, kn=False):
    """exact accumulators of the sampled batches, int64 NumPy: a [n, M, K], b [n, N, K] (kn: [n, K, N])"""
    a, b = a.cpu().numpy().astype(np.int64), b.cpu().numpy().astype(np.int64)
    return a @ (b if kn else b.transpose(0, 2, 1))


FORMS = [("bmm_i8", ops.bmm_i8, False), ("bmm_i8_kn", ops.bmm_i8_kn, True)]


@pytest.mark.parametrize("r", [1, 2], ids=["dense", "b_group2"])
def test_far_a_whole_equals_batch_chunks(r):
    """a [4100, 1024, 1024] behind an apron (6.3 GiB) crosses 2^31 and 2^32; b [4100 / r, 32, 1024] and the outputs are small.  Peak 7.5 GiB"""
    F.need(F.case("bmm-far-a").peak, "bmm far a")
    ar, a, idx = _far((B_FAR, SIDE, SIDE), 65000)
    sel = torch.tensor(idx, dtype=torch.int64, device=DEV)
    for name, op, kn in FORMS:
        b = _i8((B_FAR // r, SIDE, SMALL) if kn else (B_FAR // r, SMALL, SIDE), 65001)
        for kind in (torch.int32, torch.float32, torch.int8):
            whole = op(a, b, kind, ALPHA, b_group=r)
            _batches_equal(f"{name} {kind}", whole, lambda c, d: op(a[c:d], b[c // r:d // r], kind, ALPHA, b_group=r), B_FAR, STEP)
            want = _acc(a[sel], b[sel // r], kn)
            assert_bits_equal(whole[sel].cpu().numpy(), want.astype(np.int32) if kind == torch.int32 else ref_out(want, kind, ALPHA), f"{name} {kind}, the sampled batches")
            del whole
    b = _i8((B_FAR // r, SMALL, SIDE), 65002)
    whole = ops.bmm_i8_softmax_q8(a, b, ALPHA / 8, causal=False, b_group=r)
    _batches_equal("bmm_i8_softmax_q8", whole, lambda c, d: ops.bmm_i8_softmax_q8(a[c:d], b[c // r:d // r], ALPHA / 8, causal=False, b_group=r), B_FAR, STEP)
    assert ar.apron_intact() and ar.is_random(0, a.numel(), 65000), "a or its apron changed"
    del ar, a, b, whole
    F.release()


@pytest.mark.parametrize("m", [SMALL, 16], ids=["M32", "M16-narrow"])
def test_far_b_whole_equals_batch_chunks(m):
    """b [4100, 1024, 1024] behind an apron crosses 2^31 and 2^32, read as [B, N, K] and as [B, K, N]; a [4100, M, 1024] and the outputs are small; M = 16 takes the
    narrow kernels (bmm_i8_m16, bmm_i8_m16kn).  Peak 7.5 GiB"""
    F.need(F.case("bmm-far-b").peak, "bmm far b")
    ar, b, idx = _far((B_FAR, SIDE, SIDE), 65100)
    sel = torch.tensor(idx, dtype=torch.int64, device=DEV)
    a = _i8((B_FAR, m, SIDE), 65101)
    for name, op, kn in FORMS:
        for kind in (torch.int32, torch.int8):
            whole = op(a, b, kind, ALPHA)
            _batches_equal(f"{name} {kind}", whole, lambda c, d: op(a[c:d], b[c:d], kind, ALPHA), B_FAR, STEP)
            want = _acc(a[sel], b[sel], kn)
            assert_bits_equal(whole[sel].cpu().numpy(), want.astype(np.int32) if kind == torch.int32 else ref_out(want, kind, ALPHA), f"{name} {kind}, the sampled batches")
    whole = ops.bmm_i8_softmax_q8(a, b, ALPHA / 8)
    _batches_equal("bmm_i8_softmax_q8", whole, lambda c, d: ops.bmm_i8_softmax_q8(a[c:d], b[c:d], ALPHA / 8), B_FAR, STEP)
    assert ar.apron_intact() and ar.is_random(0, b.numel(), 65100), "b or its apron changed"
    del ar, a, b, whole
    F.release()


@pytest.mark.parametrize("kind,batches", [(torch.int8, B_FAR), (torch.float32, B_F32), (torch.int32, B_F32)], ids=["s8-4100", "f32-1030", "s32-1030"])
def test_far_out_every_batch(kind, batches):
    """K = 16: out [batches, 1024, 1024] (4.3 GB: int8 x 4100, 4 bytes x 1030) crosses 2^31 and 2^32, the operands are 67 MB.  Peak 4.8 GiB.  The op allocates the
    output, so there is no apron in front of it"""
    F.need(F.case("bmm-far-out").peak, "bmm far out")
    K = 16
    a, b = _i8((batches, SIDE, K), 65200), _i8((batches, SIDE, K), 65201)
    es = torch.empty((), dtype=kind).element_size()
    sel = torch.tensor(F.anchor_rows(SIDE * SIDE * es, batches, 2), dtype=torch.int64, device=DEV)
    for name, op, kn in FORMS:
        bb = b.transpose(1, 2).contiguous() if kn else b
        whole = op(a, bb, kind, 1.0 / 64)
        assert whole.numel() * es > F.G32
        _batches_equal(f"{name} {kind}", whole, lambda c, d: op(a[c:d], bb[c:d], kind, 1.0 / 64), batches, STEP)
        want = _acc(a[sel], bb[sel], kn)
        assert_bits_equal(whole[sel].cpu().numpy(), want.astype(np.int32) if kind == torch.int32 else ref_out(want, kind, 1.0 / 64), f"{name} {kind}, the sampled batches")
        del whole
    if kind == torch.int8:
        whole = ops.bmm_i8_softmax_q8(a, b, 1.0 / 2000)
        _batches_equal("bmm_i8_softmax_q8", whole, lambda c, d: ops.bmm_i8_softmax_q8(a[c:d], b[c:d], 1.0 / 2000), batches, STEP)
        del whole
    del a, b
    F.release()


@pytest.mark.parametrize("r", [1, 2], ids=["dense", "b_group2"])
def test_token_major_far_a_whole_equals_sequence_chunks(r):
    """a [S = 1030, 1024, h = 4, 1024] behind an apron (4.3 GB) crosses 2^31 and 2^32: entry s * 4 + head of the launch is found by the magic-number division at entry
    indices up to 4119.  b [S, 32, h / r, 1024] token-major (bmm_i8_kn: [S, 1024, h / r, 32]); out_token gives [S, 1024, 4, 32].  Peak 7 GiB.  Against chunks of 64 sequences and against the dense
    call on permuted copies of the sampled sequences"""
    F.need(F.case("bmm-token-major").peak, "bmm token-major")
    S, H = B_F32, 4
    ar, a, idx = _far((S, SIDE, H, SIDE), 65300)
    sel = torch.tensor(idx, dtype=torch.int64, device=DEV)
    for name, op, kn in FORMS:
        b = _i8((S, SIDE, H // r, SMALL) if kn else (S, SMALL, H // r, SIDE), 65301)       # token-major b: [S, N, h / r, K]; kn: [S, K, h / r, N]
        bshape = (-1, SIDE, SMALL) if kn else (-1, SMALL, SIDE)
        # bmm_i8: both kinds with and without out_token; bmm_i8_kn: each kind and each output layout once
        for kind, out_token in ((torch.int32, True), (torch.int8, False)) if kn else ((torch.int32, True), (torch.int32, False), (torch.int8, True), (torch.int8, False)):
            whole = op(a, b, kind, ALPHA, b_group=r, out_token=out_token)
            assert tuple(whole.shape) == ((S, SIDE, H, SMALL) if out_token else (S * H, SIDE, SMALL))
            view = whole if out_token else whole.view(S, H, SIDE, SMALL)
            for c, d in F.chunks(S, 64):
                part = op(a[c:d], b[c:d], kind, ALPHA, b_group=r, out_token=out_token)
                assert torch.equal(view[c:d], part if out_token else part.view(d - c, H, SIDE, SMALL)), f"{name} token-major {kind}, out_token {out_token}: sequences {c} .. {d}"
            dense = op(a[sel].permute(0, 2, 1, 3).reshape(-1, SIDE, SIDE), b[sel].permute(0, 2, 1, 3).reshape(bshape), kind, ALPHA, b_group=r)
            got = (view[sel].permute(0, 2, 1, 3) if out_token else view[sel]).reshape(-1, SIDE, SMALL)
            assert torch.equal(got, dense), f"{name} token-major {kind}, out_token {out_token}: the sampled sequences differ from the dense call on permuted copies"
            want = _acc(a[sel].permute(0, 2, 1, 3).reshape(-1, SIDE, SIDE), b[sel].permute(0, 2, 1, 3).repeat_interleave(r, 1).reshape(bshape), kn)
            assert_bits_equal(dense.cpu().numpy(), want.astype(np.int32) if kind == torch.int32 else ref_out(want, kind, ALPHA), f"{name} token-major {kind}, the sampled sequences")
            del whole, view
    b = _i8((S, SMALL, H // r, SIDE), 65302)
    whole = ops.bmm_i8_softmax_q8(a, b, ALPHA / 8, b_group=r)
    for c, d in F.chunks(S, 64):
        part = ops.bmm_i8_softmax_q8(a[c:d], b[c:d], ALPHA / 8, b_group=r)
        assert torch.equal(whole.view(S, -1)[c:d], part.view(d - c, -1)), f"bmm_i8_softmax_q8 token-major: sequences {c} .. {d}"
    assert ar.apron_intact() and ar.is_random(0, a.numel(), 65300), "a or its apron changed"
    del ar, a, b, whole
    F.release()
