"""GPU: asq_attn_extend_i8_paged through ops.attn_extend_i8_paged / Int8Attention.extend_paged (include/asq_hip_extend.h).

The entry has no arithmetic of its own, so its yardstick is the contiguous entry (tests/test_hip_attn_extend.py): tests/attn_decode_paged_child.py's scatter() lays a
contiguous cache out as pages under a seeded permutation (the pages of the sequences interleaved; every unused page, every row at or behind n_b and the pitch gap
poisoned) and the outputs are compared bit for bit, with the same max_len.

  * cases 2, 3, 5 and 8 of tests/attn_extend_ref.py at page sizes 16, 48, 80 and 256 under both signs of qk_alpha (48 and 80 do not divide the 1024- and 1088-key chunks:
    a chunk edge falls inside a page); lengths on every page seam with tokens that straddle it;
  * the device-side rules: table entries behind a sequence's last page are never read, a bad id inside the used range acts as its clamped value;
  * shared prefix pages give the bits of private copies."""
import numpy as np
import pytest
import torch

import attn_decode_paged_child as PC
import attn_extend_child as CH
import attn_extend_ref as X
from autosmoothquant_amd import ops
from bmm_ref import assert_bits_equal

pytestmark = pytest.mark.gpu
DEV = CH.DEV
PAGES = (16, 48, 80, 256)
PAGED_CASES = (1, 2, 4, 7)
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1
PV = X.PV_ALPHAS[0]


def run_paged(q, kp, vp, tab, lengths, q_len, alpha, pv, ml):
    out = ops.attn_extend_i8_paged(q, kp, vp, tab, CH._i32(lengths), alpha, pv, q_len=CH._i32(q_len), max_len=ml)
    assert out.dtype == torch.int8 and out.shape == q.shape and out.is_contiguous()
    return out.cpu().numpy()


def _both(qn, kn, vn, lengths, q_len, alpha, P, seed, what, gap=0):
    """the paged entry on the scattered cache against the contiguous entry on the original, the same max_len"""
    ml = X.max_len(lengths)
    q, k, v = CH.dev(qn, kn, vn)
    want = CH.run(q, k, v, lengths, q_len, alpha, PV, ml)
    kp, vp, tab, _ = PC.scatter(qn[:, 0], kn, vn, lengths, P, ml, seed, gap=gap, behind=I32_MAX)
    got = run_paged(q, kp, vp, tab, lengths, q_len, alpha, PV, ml)
    assert_bits_equal(got, want, what)
    assert not got[X.row_keys(lengths, q_len, qn.shape[1], ml) == 0].any() and int(np.abs(got).max()) > 0
    return got


PARAMS = [(ci, P, sign) for ci in PAGED_CASES for P in PAGES for sign in X.SIGNS]


@pytest.mark.parametrize("case,P,sign", PARAMS, ids=[f"case{ci + 1}-page{P}-{'max' if sign > 0 else 'min'}" for ci, P, sign in PARAMS])
def test_cases_equal_the_contiguous_entry(case, P, sign):
    hkv, r, sq, d, lengths, q_len = X.CASES[case]
    qn, kn, vn = X.operands(case)
    if X.chunked(case):
        assert (X.chunk(case) % P != 0) == (P in (48, 80) or (P == 256 and X.chunk(case) == 1088))
    _both(qn, kn, vn, lengths, q_len, sign * X.qk_alpha(case, 1), P, 53800 + P + case, f"case {case + 1}, page size {P}, sign {sign:+d}", gap=1 if P in (80, 256) else 0)


def _seams(P):
    return sorted({0, 1, 15, 16, 17, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 3 * P + 1})       # ..., the last page exactly full, the last page holding one row


@pytest.mark.parametrize("sign", X.SIGNS, ids=["max", "min"])
@pytest.mark.parametrize("P", PAGES)
def test_lengths_on_every_page_seam(P, sign):
    """a step of 3 tokens (q_len 3, 2, 1 in turn) ending on, one past and one short of every page edge: the new tokens' keys straddle the seam"""
    hkv, r, sq, d = (2, 4, 3, 64) if P in (16, 80) else (1, 5, 3, 128)
    lengths = _seams(P)
    q_len = [3 - b % 3 for b in range(len(lengths))]
    rng = np.random.default_rng(53850 + P)
    qn = rng.integers(-128, 128, (len(lengths), sq, hkv * r, d), dtype=np.int8)
    kn, vn = (rng.integers(-128, 128, (len(lengths), X.max_len(lengths) + 2, hkv, d), dtype=np.int8) for _ in range(2))
    _both(qn, kn, vn, lengths, q_len, sign * X.SR.alphas((1, 1, d))[1], P, 53851 + P, f"page seams, page size {P}, sign {sign:+d}", gap=1 if P == 48 else 0)


def _small():
    """r = 4, Sq = 4, D = 64, page size 16: lengths on and off the page edges"""
    lengths, q_len = [40, 16, 2, 33, 0], [4, 4, 4, 1, 3]
    rng = np.random.default_rng(53860)
    qn = rng.integers(-128, 128, (len(lengths), 4, 8, 64), dtype=np.int8)
    kn, vn = (rng.integers(-128, 128, (len(lengths), X.max_len(lengths) + 2, 2, 64), dtype=np.int8) for _ in range(2))
    return qn, kn, vn, lengths, q_len, X.SR.alphas((1, 1, 64))[1], X.max_len(lengths)


def test_table_entries_behind_the_last_page_are_never_read():
    qn, kn, vn, lengths, q_len, alpha, ml = _small()
    q, k, v = CH.dev(qn, kn, vn)
    want = CH.run(q, k, v, lengths, q_len, alpha, PV, ml)
    for behind in (-1, None, I32_MIN, I32_MAX):
        kp, vp, tab, host = PC.scatter(qn[:, 0], kn, vn, lengths, 16, ml, 53861, behind=0)
        bad = kp.shape[0] if behind is None else behind        # num_pages: the first id past the pool
        for b, n in enumerate(lengths):
            host[b, -(-n // 16):] = bad
        full = torch.from_numpy(host).to(DEV)
        assert_bits_equal(run_paged(q, kp, vp, full[:, :tab.shape[1]], lengths, q_len, alpha, PV, ml), want, f"entries behind ceil(n_b / P) set to {bad}")


def test_a_bad_entry_inside_the_used_range_acts_as_its_clamped_value():
    qn, kn, vn, lengths, q_len, alpha, ml = _small()
    q, = CH.dev(qn)
    kp, vp, tab, host = PC.scatter(qn[:, 0], kn, vn, lengths, 16, ml, 53862, behind=0)
    num_pages = kp.shape[0]
    for bad, clamped in ((-1, 0), (I32_MIN, 0), (num_pages, num_pages - 1), (I32_MAX, num_pages - 1)):
        a, c = host.copy(), host.copy()
        a[0, 1], c[0, 1] = bad, clamped                         # sequence 0's second page
        a[3, 2], c[3, 2] = bad, clamped                         # sequence 3's last page, which holds one key
        ta, tc = (torch.from_numpy(x).to(DEV)[:, :tab.shape[1]] for x in (a, c))
        assert_bits_equal(run_paged(q, kp, vp, ta, lengths, q_len, alpha, PV, ml), run_paged(q, kp, vp, tc, lengths, q_len, alpha, PV, ml), f"a table entry of {bad} against {clamped}")


def test_shared_prefix_pages_give_the_bits_of_private_copies():
    qn, kn, vn, lengths, q_len, alpha, ml = _small()
    kn, vn = kn.copy(), vn.copy()
    kn[3, :32], vn[3, :32] = kn[0, :32], vn[0, :32]             # sequences 0 and 3 share a prefix of two pages
    q, k, v = CH.dev(qn, kn, vn)
    want = CH.run(q, k, v, lengths, q_len, alpha, PV, ml)
    kp, vp, tab, host = PC.scatter(qn[:, 0], kn, vn, lengths, 16, ml, 53863, behind=-1, share=(0, 3, 2))
    assert host[3, :2].tolist() == host[0, :2].tolist() and host[3, 2] != host[0, 2]
    assert_bits_equal(run_paged(q, kp, vp, tab, lengths, q_len, alpha, PV, ml), want, "shared prefix pages")
    kp2, vp2, tab2, host2 = PC.scatter(qn[:, 0], kn, vn, lengths, 16, ml, 53863, behind=-1)
    assert not set(host2[3, :3].tolist()) & set(host2[0, :3].tolist())
    assert_bits_equal(run_paged(q, kp2, vp2, tab2, lengths, q_len, alpha, PV, ml), want, "private copies of the prefix")
