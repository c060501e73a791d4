"""Guard bands for the entries of include/asq_hip_extend.h, with the arena plumbing of tests/test_hip_guardband.py (`Run`, `same_bits`, the value generators), in the
shape of tests/test_hip_guardband_decode.py and tests/test_hip_guardband_paged.py.

asq_attn_extend_i8: q, both caches (as [B, max_len + 2 rows] regions: the pitch is wider than max_len rows), kv_len and q_len are input regions, out an output region.
asq_attn_extend_i8_paged: q, both pools (a page pitch one row wider than a page), the block table (its row stride wider than its width, ids far outside the pool behind
every sequence's last page), kv_len and q_len are inputs, out the output.  The raw call returns ASQ_OK, writes the bytes of the ordinary ops call -- the rows of padded
tokens as zeros -- leaves every guard and every input as it was and gives the same bytes under both flank poisons.  kv_len and q_len hold entries above their range and
below 0: a kernel that trusted them would read a flank of a cache or of q, or write one of out.  The shapes take every ceil(D / 64) of 1 to 4, one to three token groups
with a last group that is partly filled, the one-pass and the chunked path.
An empty problem (B, Sq, Hq or Hkv of 0) leaves every output byte.  CASES is the table tests/test_attn_extend_cpu.py checks against _lib.EXTEND_SIGNATURES."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from test_hip_guardband import ASQ_OK, I8, Case, Run, _dev, ri8, same_bits
from test_hip_guardband_paged import BAD_IDS, _table

pytestmark = pytest.mark.gpu

EXTEND, PAGED = "asq_attn_extend_i8", "asq_attn_extend_i8_paged"
ALPHAS = (0.0009, 1.0 / 127)
# (B, Sq, Hq, Hkv, D, max_len, kv_len, q_len or None): the second and the last are chunked (16 rows: 1024 keys per chunk); q_len above Sq, 0 and below 0; Sq = 3 at
# r = 8 and Sq = 7 at r = 3 leave the last token group partly filled; a sequence with more tokens than keys
SHAPES = [(2, 4, 4, 2, 64, 40, [49, 17], None), (3, 3, 8, 1, 128, 1100, [1100, -3, 1029], [3, 2, 1 << 30]), (4, 2, 2, 2, 16, 5, [1, 0, 5, 3], [2, 2, -7, 0]),
          (2, 7, 6, 2, 192, 70, [70, 3], [4, 7]), (1, 2, 16, 1, 256, 1100, [1100], None)]
PAGE = {64: 16, 128: 48, 16: 16, 192: 32, 256: 64}     # the page size per shape, by head dim
ARENA_BYTES = 64 << 20
CASES = []

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def _lens(kv_len, q_len):
    dev = _dev()
    return torch.tensor(kv_len, dtype=torch.int32, device=dev), None if q_len is None else torch.tensor(q_len, dtype=torch.int32, device=dev)


def _padded(B, Sq, ml, kv_len, q_len):
    """[B, Sq] bool: the tokens whose output row is zeros by the per-token rule"""
    z = torch.zeros((B, Sq), dtype=torch.bool)
    for b in range(B):
        n = min(max(kv_len[b], 0), ml)
        m = Sq if q_len is None else min(max(q_len[b], 0), Sq)
        for s in range(Sq):
            z[b, s] = s >= m or n - m + s + 1 <= 0
    return z


def _extend(B, Sq, Hq, Hkv, D, ml, kv_len, q_len):
    def make():
        from autosmoothquant_amd import ops
        rows = ml + 2
        q, k, v = ri8((B, Sq, Hq, D), "ext-q"), ri8((B, rows, Hkv * D), "ext-k"), ri8((B, rows, Hkv * D), "ext-v")
        n, m = _lens(kv_len, q_len)

        def call(r):
            pq, pk, pv, pn = r.inp("q", q), r.inp("k_cache", k), r.inp("v_cache", v), r.inp("kv_len", n)
            pm = None if m is None else r.inp("q_len", m)
            po = r.out("out", (B, Sq, Hq, D), I8)
            return L.lib().asq_attn_extend_i8(pq, pk, pv, pn, pm, po, B, Sq, Hq, Hkv, D, rows * Hkv * D, ml, *ALPHAS, r.stream)

        def ref():
            return ops.attn_extend_i8(q, k.view(B, rows, Hkv, D)[:, :ml], v.view(B, rows, Hkv, D)[:, :ml], n, *ALPHAS, q_len=m)
        return call, ref, _padded(B, Sq, ml, kv_len, q_len)
    return make


def _paged(B, Sq, Hq, Hkv, D, ml, kv_len, q_len):
    def make():
        from autosmoothquant_amd import ops
        P = PAGE[D]
        width = -(-ml // P)
        stride, num_pages, rows = width + 3, B * width + 2, P + 1
        q, k, v = ri8((B, Sq, Hq, D), "xpg-q"), ri8((num_pages, rows, Hkv * D), "xpg-k"), ri8((num_pages, rows, Hkv * D), "xpg-v")
        used = [-(-max(0, min(x, ml)) // P) for x in kv_len]
        tab = _table(B, width, stride, used, num_pages, 53700 + D, lambda i: (num_pages, *BAD_IDS)[i % 4]).to(_dev())
        n, m = _lens(kv_len, q_len)

        def call(r):
            pq, pk, pv, pt, pn = r.inp("q", q), r.inp("k_pool", k), r.inp("v_pool", v), r.inp("block_table", tab), r.inp("kv_len", n)
            pm = None if m is None else r.inp("q_len", m)
            po = r.out("out", (B, Sq, Hq, D), I8)
            return L.lib().asq_attn_extend_i8_paged(pq, pk, pv, pt, pn, pm, po, B, Sq, Hq, Hkv, D, num_pages, P, rows * Hkv * D, stride, ml, *ALPHAS, r.stream)

        def ref():
            return ops.attn_extend_i8_paged(q, k.view(num_pages, rows, Hkv, D)[:, :P], v.view(num_pages, rows, Hkv, D)[:, :P], tab[:, :width], n, *ALPHAS, q_len=m, max_len=ml)
        return call, ref, _padded(B, Sq, ml, kv_len, q_len)
    return make


def _empty(entry, dims):
    def make():
        def call(r):
            z = torch.ones((256,), dtype=torch.float16, device=_dev())
            px, pn = r.inp("x", z), r.inp("n", torch.zeros((64,), dtype=torch.int32, device=_dev()))
            po = r.out("o0", (256,), torch.uint8, 256)
            if entry == EXTEND:
                return L.lib().asq_attn_extend_i8(px, px, px, pn, pn, po, *dims, 0, 8, *ALPHAS, r.stream)
            return L.lib().asq_attn_extend_i8_paged(px, px, px, pn, pn, pn, po, *dims, 4, 16, 0, 2, 8, *ALPHAS, r.stream)
        return call, None, None
    return make


for _entry, _make in ((EXTEND, _extend), (PAGED, _paged)):
    for _s in SHAPES:
        CASES.append(Case(_entry, f"{_entry}-B{_s[0]}S{_s[1]}H{_s[2]}x{_s[3]}D{_s[4]}-max{_s[5]}", _make(*_s)))
    for _cid, _dims in (("B0", (0, 3, 4, 2, 16)), ("Sq0", (2, 0, 4, 2, 16)), ("Hq0", (2, 3, 0, 0, 16)), ("Hkv0", (2, 3, 4, 0, 16))):
        CASES.append(Case(_entry, f"{_entry}-empty-{_cid}", _empty(_entry, _dims)))
WRITERS = [c for c in CASES if "-empty-" not in c.id]
NOTHING = [c for c in CASES if "-empty-" in c.id]


def _runs(c, call):
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = call(run)
        assert rc == ASQ_OK, (c.id, rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        yield poison, run, run.results()
        rep = run.arena.check()
        assert rep.ok, f"{c.id} (flank 0x{poison:02X}): {rep}"


@pytest.mark.parametrize("c", WRITERS, ids=[c.id for c in WRITERS])
def test_extend_writes_only_out_and_reads_no_flank(c):
    call, ref, padded = c.make()
    want = ref()
    torch.cuda.synchronize()
    assert int(want.abs().max()) > 0 and not want[padded.to(want.device)].any()
    got = []
    for poison, run, res in _runs(c, call):
        assert same_bits(res["out"], want), f"{c.id} (flank 0x{poison:02X}): out differs from the ops call"
        assert not res["out"][padded.to(res["out"].device)].any(), f"{c.id} (flank 0x{poison:02X}): a padded token's row is not zeros"
        got.append(res["out"])
    assert same_bits(got[0], got[1])


@pytest.mark.parametrize("c", NOTHING, ids=[c.id for c in NOTHING])
def test_nothing_to_do_leaves_every_output_byte(c):
    call, _, _ = c.make()
    for poison, run, _res in _runs(c, call):
        for k, (reg, _, _) in run.outs.items():
            assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), f"{c.id}: an empty call wrote into '{k}'"
