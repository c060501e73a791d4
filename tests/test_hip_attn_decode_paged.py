"""GPU: asq_attn_decode_i8_paged through ops.attn_decode_i8_paged / Int8Attention.decode_paged (include/asq_hip_paged.h).

The entry has no arithmetic of its own, so its yardstick is the contiguous entry: tests/attn_decode_paged_child.py's scatter() lays a contiguous cache out as pages
under a seeded permutation (the pages of the sequences interleaved; every unused page, every row at or behind n_b and the pitch gap poisoned with the key that would
win its row outright) and the outputs are compared bit for bit.

  * bit-equal to ops.attn_decode_i8 on the contiguous original with the same max_len: page sizes 16 .. 256 (48 and 80 do not divide the chunks: a chunk edge falls
    inside a page), r of 1, 4, 5, 7 and 16, D of 16 .. 256, the one-pass and the chunked path (both signs of qk_alpha), lengths on every page seam;
  * exact families straight through the paged entry, independent of the contiguous kernel: the key-position walk and the two weights at page sizes 16 and 80, the
    uniform softmax at 32;
  * the device-side rules: table entries behind a sequence's last page are never read, a bad id inside the used range acts as its clamped value, kv_len above
    max_len / negative / NULL, a table row stride wider than the table, a page-pitch gap;
  * shared pages; the 4-wave and 16-wave kernels in a child process each;
  * the gate: at the bench shape with page size 16 the paged launch beats gathering the pages into contiguous caches and launching the contiguous entry."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import attn_decode_paged_child as PC
import attn_decode_ref as R
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal, medians_us, ref_out

pytestmark = pytest.mark.gpu
DEV = PC.DEV
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGES = (16, 32, 48, 64, 80, 128, 256)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


def _random(B, hkv, r, d, rows, seed):
    rng = np.random.default_rng(seed)
    q = rng.integers(-128, 128, (B, hkv * r, d), dtype=np.int8)
    k, v = (rng.integers(-128, 128, (B, rows, hkv, d), dtype=np.int8) for _ in range(2))
    return q, k, v


def _contiguous(qn, kn, vn, lengths, alpha, pv, ml, kv_len="lengths"):
    q, k, v = PC.dev(qn, kn, vn)
    if isinstance(kv_len, str):
        kv_len = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    return ops.attn_decode_i8(q, k[:, :ml], v[:, :ml], kv_len, alpha, pv, max_len=ml).cpu().numpy()


def _both(qn, kn, vn, lengths, alpha, P, seed, what, gap=0, pv=R.PV_ALPHAS[0]):
    """the paged entry on the scattered cache against the contiguous entry on the original, the same max_len"""
    ml = R.max_len(lengths)
    want = _contiguous(qn, kn, vn, lengths, alpha, pv, ml)
    kp, vp, tab, _ = PC.scatter(qn, kn, vn, lengths, P, ml, seed, gap=gap, behind=I32_MAX)
    got = PC.run_paged(PC.dev(qn)[0], kp, vp, tab, lengths, alpha, pv, ml)
    assert_bits_equal(got, want, what)
    for b, n in enumerate(lengths):
        if n == 0:
            assert not got[b].any(), f"{what}: a sequence without keys is not all zeros"
    assert int(np.abs(got).max()) > 0
    return got


def _seams(P):
    return sorted({0, 1, 15, 16, 17, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 3 * P + 1})       # ..., the last page exactly full, the last page holding one row


# page size -> the (r, D) it runs on the one-pass path: every r of 1, 4, 5, 16 and every D of 16, 64, 128, 192, 256 at least once
ONE_PASS = {16: [(1, 16), (16, 128)], 32: [(4, 64)], 48: [(5, 128), (16, 256)], 64: [(16, 192)], 80: [(1, 256), (4, 128)], 128: [(5, 64)], 256: [(16, 16), (4, 192)]}


@pytest.mark.parametrize("P,r,d", [(P, r, d) for P in PAGES for r, d in ONE_PASS[P]])
def test_one_pass_equals_the_contiguous_entry_on_every_page_seam(P, r, d):
    lengths = _seams(P)
    assert max(lengths) <= R.chunk(r, R.max_len(lengths))
    qn, kn, vn = _random(len(lengths), 2, r, d, R.max_len(lengths) + 2, 52900 + P + r)
    _both(qn, kn, vn, lengths, R.SR.alphas((1, 1, d))[1], P, 52901 + P, f"page size {P}, r {r}, D {d}, one pass", gap=1 if P in (32, 80, 256) else 0)


# (r, D, lengths): just over one and two chunks of 1024 at r = 16; r = 5 just over its chunk of 3264 (with 2310 keys next to it: one pass); r = 7 just over its chunk of
# 2304; the last with ND = 4
CHUNKED = [(16, 64, [1030, 2055]), (5, 128, [3270, 2310]), (7, 128, [2310, 17]), (16, 256, [1030])]


# the ND = 4 form at the two page sizes that do not divide its chunk, the others at every page size
CHUNKED_PARAMS = [(P, s, sign) for s in CHUNKED for P in PAGES if s[1] != 256 or P in (48, 80) for sign in (1, -1)]


@pytest.mark.parametrize("P,shape,sign", CHUNKED_PARAMS, ids=[f"page{P}-r{s[0]}d{s[1]}-{'max' if sign > 0 else 'min'}" for P, s, sign in CHUNKED_PARAMS])
def test_chunked_equals_the_contiguous_entry(P, shape, sign):
    r, d, lengths = shape
    ml = R.max_len(lengths)
    C = R.chunk(r, ml)
    assert max(lengths) > C and (r != 16 or (C % P != 0) == (P in (48, 80)))       # 1024 keys: a chunk edge falls inside a page of 48 or 80 (2304 = 48 * 48 and 3264 = 48 * 68: of 80 only)
    qn, kn, vn = _random(len(lengths), 1, r, d, ml + 2, 52950 + P + r)
    _both(qn, kn, vn, lengths, sign * R.SR.alphas((1, 1, d))[1], P, 52951 + P, f"page size {P}, r {r}, D {d}, chunks of {C}, sign {sign:+d}", gap=1 if P == 80 else 0)


@pytest.mark.parametrize("P", [16, 80])
@pytest.mark.parametrize("i", [0, 1], ids=[f"kv{s[0]}x{s[1]}d{s[2]}" for s in R.WALK[:2]])
def test_key_position_walk_is_exact_through_the_paged_entry(i, P):
    PC.walk(i, 8, P)


@pytest.mark.parametrize("neg", [False, True], ids=["max", "min"])
@pytest.mark.parametrize("P", [16, 80])
@pytest.mark.parametrize("i", [0, 1], ids=[f"kv{s[0]}x{s[1]}d{s[2]}" for s in R.WALK[:2]])
def test_two_weights_are_exact_through_the_paged_entry(i, P, neg):
    PC.two_weights(i, neg, P)


def test_uniform_softmax_is_exact_through_the_paged_entry():
    made = R.uniform_case()
    qn, kn, vn, lengths = made[:4]
    r = qn.shape[1] // kn.shape[2]
    s = np.stack([vn[b, :n].astype(np.int64).sum(axis=0) for b, n in enumerate(lengths)]).repeat(r, axis=1)
    PC.exact(made, 32, lambda pv: ref_out(s, torch.int8, pv), "uniform softmax", 52820)


def _small():
    """r = 4, D = 64, page size 16: lengths on and off the page edges"""
    lengths = [40, 16, 1, 33, 0]
    qn, kn, vn = _random(len(lengths), 2, 4, 64, R.max_len(lengths) + 2, 52830)
    return qn, kn, vn, lengths, R.SR.alphas((1, 1, 64))[1], R.max_len(lengths)


def test_table_entries_behind_the_last_page_are_never_read():
    qn, kn, vn, lengths, alpha, ml = _small()
    pv = R.PV_ALPHAS[0]
    want = _contiguous(qn, kn, vn, lengths, alpha, pv, ml)
    q, = PC.dev(qn)
    for behind in (-1, None, I32_MIN, I32_MAX):
        kp, vp, tab, host = PC.scatter(qn, kn, vn, lengths, 16, ml, 52831, behind=0)
        bad = kp.shape[0] if behind is None else behind        # num_pages: the first id past the pool
        for b, n in enumerate(lengths):
            host[b, -(-n // 16):] = bad
        full = torch.from_numpy(host).to(DEV)
        assert_bits_equal(PC.run_paged(q, kp, vp, full[:, :tab.shape[1]], lengths, alpha, pv, ml), want, f"entries behind ceil(n_b / P) set to {bad}")


def test_a_bad_entry_inside_the_used_range_acts_as_its_clamped_value():
    qn, kn, vn, lengths, alpha, ml = _small()
    pv = R.PV_ALPHAS[0]
    q, = PC.dev(qn)
    kp, vp, tab, host = PC.scatter(qn, kn, vn, lengths, 16, ml, 52832)
    num_pages, width = kp.shape[0], tab.shape[1]
    for bad, clamped in ((-7, 0), (I32_MIN, 0), (num_pages, num_pages - 1), (I32_MAX, num_pages - 1)):
        outs = []
        for value in (bad, clamped):
            h = host.copy()
            h[0, 1], h[3, 2] = value, value                     # sequence 0's second page, sequence 3's last (one valid row)
            outs.append(PC.run_paged(q, kp, vp, torch.from_numpy(h).to(DEV)[:, :width], lengths, alpha, pv, ml))
        assert_bits_equal(outs[0], outs[1], f"table entry {bad} against {clamped}")
        if host[0, 1] != clamped:                               # (the entry matters: another page's keys)
            assert (outs[0][0] != PC.run_paged(q, kp, vp, tab, lengths, alpha, pv, ml)[0]).any()


def test_kv_len_variations_on_pages():
    case, P = 2, 48
    qn, kn, vn, lengths = R.operands(case)
    ml, alpha, pv = R.max_len(lengths), R.qk_alpha(case, 1), R.PV_ALPHAS[0]
    q, = PC.dev(qn)
    full = (ml,) * len(lengths)
    kp, vp, tab, _ = PC.scatter(qn, kn, vn, full, P, ml, 52833, behind=-1)
    want = _contiguous(qn, kn, vn, full, alpha, pv, ml, kv_len=None)
    assert_bits_equal(PC.run_paged(q, kp, vp, tab, full, alpha, pv, ml, kv_len=None), want, "kv_len None: max_len keys each")
    assert_bits_equal(PC.run_paged(q, kp, vp, tab, full, alpha, pv, ml), want, "kv_len = max_len")
    wild = torch.tensor([ml + 1, -5, lengths[2], 1 << 30, I32_MIN], dtype=torch.int32, device=DEV)
    clamped = [ml, 0, lengths[2], ml, 0]
    got = PC.run_paged(q, kp, vp, tab, None, alpha, pv, ml, kv_len=wild)
    assert_bits_equal(got, _contiguous(qn, kn, vn, clamped, alpha, pv, ml), "kv_len outside 0 .. max_len against its clamped value on the contiguous entry")
    assert not got[1].any() and not got[4].any()
    q4 = q.view(q.shape[0], 1, q.shape[1], q.shape[2])          # [B, 1, Hq, D] in, the same shape out, the same bytes; the module
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    out4 = Int8Attention(alpha, pv).to(DEV).decode_paged(q4, kp, vp, tab, wild, max_len=ml)
    assert out4.shape == q4.shape and np.array_equal(out4.cpu().numpy().reshape(qn.shape), got)
    assert tab.stride(0) == tab.shape[1] + PC.SPARE_COLS        # (every table here is a view of a wider one: the row stride is not the width)


def test_shared_pages_give_the_bits_of_private_copies():
    P, r, d = 16, 4, 64
    lengths = [50, 45]
    qn, kn, vn = _random(2, 2, r, d, R.max_len(lengths) + 2, 52834)
    kn[1, :2 * P], vn[1, :2 * P] = kn[0, :2 * P], vn[0, :2 * P]            # a shared prefix of two pages
    alpha, pv, ml = R.SR.alphas((1, 1, d))[1], R.PV_ALPHAS[0], R.max_len(lengths)
    private = _both(qn, kn, vn, lengths, alpha, P, 52835, "private copies")
    kp, vp, tab, host = PC.scatter(qn, kn, vn, lengths, P, ml, 52835, share=(0, 1, 2))
    assert list(host[1, :2]) == list(host[0, :2]) and host[1, 2] != host[0, 2]
    assert_bits_equal(PC.run_paged(PC.dev(qn)[0], kp, vp, tab, lengths, alpha, pv, ml), private, "two sequences naming the same two pages")


@pytest.mark.parametrize("nw", [4, 16])
def test_the_4_wave_and_16_wave_paged_kernels_in_a_child_process(nw):
    """ASQ_DECODE_WAVES is latched on first use: tests/attn_decode_paged_child.py runs the walk for its own number of waves at page size 16 in a fresh process.  A
    child that ends by a signal or the time limit fails this test; nothing is tried again"""
    env = dict(os.environ, ASQ_DECODE_WAVES=str(nw))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_decode_paged_child.py"), str(nw)], env=env, capture_output=True, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, f"the {nw}-wave child returned {r.returncode}: {r.stdout[-1500:]} {r.stderr[-1500:]}"
    assert f"{nw} waves: all passed" in r.stdout


def test_gate_faster_than_gathering_the_pages_plus_the_contiguous_launch():
    """16 sequences x 32 / 8 heads x d = 128, 4096 keys each in pages of 16 scattered over the pool by a seeded permutation: (p) the paged launch against (g)
    index_select of both pools into contiguous caches followed by the contiguous launch, what a paged caller paid before.  (p) / (a), the contiguous launch alone on
    caches gathered outside the timer, is printed."""
    from autosmoothquant_amd.layers.nn.attention import Int8Attention
    B, Hq, Hkv, D, n, P, nrot = 16, 32, 8, 128, 4096, 16, 3
    att = Int8Attention(R.SR.alphas((1, 1, D))[1], 1.0 / 127, causal=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(52840)
    pages = B * n // P
    sets = []
    for i in range(nrot):      # 3 x 2 x 64 MiB of pools: the rotation walks past the Infinity Cache
        q = torch.randint(-128, 128, (B, 1, Hq, D), dtype=torch.int8, device=DEV, generator=g)
        kp, vp = (torch.randint(-128, 128, (pages, P, Hkv, D), dtype=torch.int8, device=DEV, generator=g) for _ in range(2))
        tab = torch.randperm(pages, generator=torch.Generator().manual_seed(52841 + i)).to(torch.int32).view(B, n // P).to(DEV)
        flat = tab.flatten()
        sets.append((q, kp, vp, tab, flat, kp.index_select(0, flat).view(B, n, Hkv, D), vp.index_select(0, flat).view(B, n, Hkv, D)))
    kv_len = torch.full((B,), n, dtype=torch.int32, device=DEV)
    p = lambda i: att.decode_paged(sets[i][0], sets[i][1], sets[i][2], sets[i][3], kv_len, max_len=n)  # noqa: E731
    gth = lambda i: att.decode(sets[i][0], sets[i][1].index_select(0, sets[i][4]).view(B, n, Hkv, D), sets[i][2].index_select(0, sets[i][4]).view(B, n, Hkv, D), kv_len, max_len=n)  # noqa: E731
    a = lambda i: att.decode(sets[i][0], sets[i][5], sets[i][6], kv_len, max_len=n)  # noqa: E731
    assert torch.equal(p(0), gth(0)) and torch.equal(p(0), a(0))
    # (p) and (g) read the same pools: in one iteration (g) takes the set two ahead of (p)'s, so neither finds its pool warm from the other's call just before
    tp, tg, ta = medians_us([p, lambda i: gth((i + 2) % nrot), lambda i: a((i + 1) % nrot)], nrot)
    print(f"paged launch {tp:.1f} us, gather + contiguous launch {tg:.1f} us, contiguous launch alone {ta:.1f} us: paged / contiguous = {tp / ta:.2f}")
    del sets, p, gth, a
    torch.cuda.empty_cache()                                    # 0.8 GB of operands: the allocator's cache goes back, as after the other timed tests
    assert tp < tg, f"the paged launch ({tp:.1f} us) is not faster than gathering the pages + the contiguous launch ({tg:.1f} us)"
