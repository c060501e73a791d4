"""Guard bands for the entries of include/asq_hip_paged.h, with the arena plumbing of tests/test_hip_guardband.py (`Run`, `same_bits`, the value generators), in the
shape of tests/test_hip_guardband_decode.py.

asq_attn_decode_i8_paged: q, both pools (with a page pitch one row wider than a page), the block table (its row stride wider than its width) and kv_len are input
regions, out an output region.  The raw call returns ASQ_OK, writes the bytes of the ordinary ops.attn_decode_i8_paged call, leaves every guard and every input as it
was and gives the same bytes under both flank poisons.  kv_len holds entries above max_len and below 0, and the table holds ids far outside the pool behind every
sequence's last page: a kernel that trusted either would read a flank.
asq_rope_quantize_qkv_paged: q, k, v as the three slices of one fused input region, the tables, pos and the block table as inputs, q8 and the two whole pools as outputs.
Every pool byte outside the rows the table names for positions pos[b] .. pos[b] + S - 1 stays at the arena's pattern, the written rows and q8 equal
ops.rope_quantize_qkv called per sequence, and a token out of range (its position, or its page id) writes no pool byte and a zero q8 row.
An empty problem leaves every output byte.  CASES is the table tests/test_paged_decode_cpu.py checks against _lib.PAGED_SIGNATURES."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from test_hip_guardband import ASQ_OK, CODE, FLOATS, I8, NAME, Case, Run, _dev, esize, ri8, rnd, same_bits

pytestmark = pytest.mark.gpu

DECODE, APPEND = "asq_attn_decode_i8_paged", "asq_rope_quantize_qkv_paged"
ALPHAS = (0.0009, 1.0 / 127)
SCALES = (0.37, 0.11, 0.73)
# (B, Hq, Hkv, D, page_size, max_len, kv_len): every ceil(D / 64) of 1 to 4; the second and the last are chunked (16 rows: 1024 keys per chunk), the second with a page size
# that does not divide the chunk
DECODE_SHAPES = [(2, 4, 2, 64, 16, 40, [49, 17]), (3, 16, 1, 128, 48, 1100, [1100, -3, 1029]), (4, 2, 2, 16, 16, 1, [1, 0, 5, 1]), (2, 6, 2, 192, 32, 70, [70, 33]),
                 (1, 16, 1, 256, 64, 1100, [1100])]
# (B, S, Hq, Hkv, D, page_size, T, max_len, pos): -1, 100 and a run that crosses min(T, max_len) are out of range in part or in whole
APPEND_SHAPES = [(1, 1, 1, 1, 16, 16, 6, 16, [0]), (3, 1, 8, 2, 128, 16, 40, 30, [15, 0, 16]), (4, 5, 4, 4, 64, 16, 40, 44, [14, -1, 38, 100]), (2, 37, 5, 1, 48, 48, 90, 96, [13, 47])]
BAD_IDS = (-1, -(1 << 31), (1 << 31) - 1)
ARENA_BYTES = 64 << 20
CASES = []

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def _table(B, width, stride, used, num_pages, seed, fill):
    """int32 [B, stride]: sequence b's first used[b] entries are distinct pages of a seeded permutation (interleaved over the sequences), every other entry is `fill(i)`"""
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(num_pages, generator=g).tolist()
    t = torch.tensor([fill(i) for i in range(B * stride)], dtype=torch.int32).view(B, stride)
    for j in range(max(used, default=0)):
        for b in range(B):
            if j < used[b]:
                t[b, j] = perm.pop()
    return t


def _decode(B, Hq, Hkv, D, P, ml, kv_len):
    def make():
        from autosmoothquant_amd import ops
        width = -(-ml // P)
        stride, num_pages, rows = width + 3, B * width + 2, P + 1
        q, k, v = ri8((B, Hq, D), "pg-q"), ri8((num_pages, rows, Hkv * D), "pg-k"), ri8((num_pages, rows, Hkv * D), "pg-v")
        used = [-(-max(0, min(n, ml)) // P) for n in kv_len]
        tab = _table(B, width, stride, used, num_pages, 52700 + D, lambda i: (num_pages, *BAD_IDS)[i % 4]).to(_dev())
        n = torch.tensor(kv_len, dtype=torch.int32, device=_dev())

        def call(r):
            pq, pk, pv, pt, pn = r.inp("q", q), r.inp("k_pool", k), r.inp("v_pool", v), r.inp("block_table", tab), r.inp("kv_len", n)
            po = r.out("out", (B, Hq, D), I8)
            return L.lib().asq_attn_decode_i8_paged(pq, pk, pv, pt, pn, po, B, Hq, Hkv, D, num_pages, P, rows * Hkv * D, stride, ml, *ALPHAS, r.stream)

        def ref():
            return ops.attn_decode_i8_paged(q, k.view(num_pages, rows, Hkv, D)[:, :P], v.view(num_pages, rows, Hkv, D)[:, :P], tab[:, :width], n, *ALPHAS, max_len=ml)
        return call, ref
    return make


def _append(dt, B, S, Hq, Hkv, D, P, T, ml, pos):
    def make():
        from autosmoothquant_amd import ops
        fused = rnd(dt, (B, S, (Hq + 2 * Hkv) * D), "pg-qkv", scale=20.0)
        cos, sin = rnd(dt, (T, D // 2), "pg-cos", scale=0.5), rnd(dt, (T, D // 2), "pg-sin", scale=0.5)
        p = torch.tensor(pos, dtype=torch.int32, device=_dev())
        ld = (Hq + 2 * Hkv) * D
        q, k, v = (fused[..., a * D:b * D].unflatten(-1, (b - a, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))
        width = -(-ml // P)
        num_pages = B * width + 1
        host = _table(B, width, width, [width] * B, num_pages, 52710 + D, lambda i: 0)
        if B > 1:
            host[1, 0] = num_pages                              # a page id outside the pool: sequence 1's tokens of page 0 are skipped
        tab = host.to(_dev())

        def call(r):
            px, pc, ps, pp, pt = r.inp("qkv", fused), r.inp("cos", cos), r.inp("sin", sin), r.inp("pos", p), r.inp("block_table", tab)
            pq8 = r.out("q8", (B, S, Hq, D), I8)
            pk, pv = r.out("k_pool", (num_pages, P, Hkv * D), I8), r.out("v_pool", (num_pages, P, Hkv * D), I8)
            return L.lib().asq_rope_quantize_qkv_paged(px, px + Hq * D * esize(dt), px + (Hq + Hkv) * D * esize(dt), ld, ld, ld, CODE[dt], pc, ps, T, pp, pt,
                                                       pq8, pk, pv, num_pages, P, 0, width, ml, *SCALES, B, S, Hq, Hkv, D, r.stream)

        def ref():
            """-> (q8 [B, S, Hq, D] with zero rows for the skipped tokens, [(page, row, k8 [Hkv * D], v8 [Hkv * D])] for the written ones), from the single-position op"""
            q8 = torch.zeros((B, S, Hq, D), dtype=I8, device=_dev())
            written = []
            lim = min(T, ml)
            for b in range(B):
                for s in range(S):
                    c = pos[b] + s
                    if pos[b] < 0 or c >= lim or not 0 <= int(host[b, c // P]) < num_pages:
                        continue
                    a, k8, v8 = ops.rope_quantize_qkv(q[b:b + 1, s:s + 1], k[b:b + 1, s:s + 1], v[b:b + 1, s:s + 1], cos, sin, *SCALES, pos=c)
                    q8[b, s] = a[0, 0]
                    written.append((int(host[b, c // P]), c % P, k8.reshape(-1), v8.reshape(-1)))
            return q8, written
        return call, ref
    return make


def _empty(entry, dims):
    def make():
        def call(r):
            z = torch.ones((256,), dtype=torch.float16, device=_dev())
            px, pn = r.inp("x", z), r.inp("n", torch.zeros((64,), dtype=torch.int32, device=_dev()))
            outs = [r.out(n, (256,), torch.uint8, 256) for n in ("o0", "o1", "o2")]
            if entry == DECODE:
                return L.lib().asq_attn_decode_i8_paged(px, px, px, pn, pn, outs[0], *dims, 4, 16, 0, 2, 8, *ALPHAS, r.stream)
            return L.lib().asq_rope_quantize_qkv_paged(px, px, px, 0, 0, 0, L.ASQ_F16, px, px, 8, pn, pn, *outs, 4, 16, 0, 2, 8, *SCALES, *dims, r.stream)
        return call, None
    return make


for _s in DECODE_SHAPES:
    CASES.append(Case(DECODE, f"{DECODE}-B{_s[0]}H{_s[1]}x{_s[2]}D{_s[3]}-page{_s[4]}-max{_s[5]}", _decode(*_s)))
for _dt in FLOATS:
    for _s in APPEND_SHAPES:
        CASES.append(Case(APPEND, f"{APPEND}-{NAME[_dt]}-B{_s[0]}S{_s[1]}H{_s[2]}+2x{_s[3]}D{_s[4]}-page{_s[5]}", _append(_dt, *_s)))
for _cid, _dims in (("B0", (0, 4, 2, 16)), ("Hq0", (2, 0, 0, 16))):
    CASES.append(Case(DECODE, f"{DECODE}-empty-{_cid}", _empty(DECODE, _dims)))
for _cid, _dims in (("B0", (0, 3, 4, 2, 16)), ("S0", (2, 0, 4, 2, 16))):
    CASES.append(Case(APPEND, f"{APPEND}-empty-{_cid}", _empty(APPEND, _dims)))
DECODES = [c for c in CASES if c.entry == DECODE and "-empty-" not in c.id]
APPENDS = [c for c in CASES if c.entry == APPEND and "-empty-" not in c.id]
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


@pytest.mark.parametrize("c", DECODES, ids=[c.id for c in DECODES])
def test_paged_decode_writes_only_out_and_reads_no_flank(c):
    call, ref = c.make()
    want = ref()
    torch.cuda.synchronize()
    assert int(want.abs().max()) > 0
    got = []
    for poison, run, res in _runs(c, call):
        assert same_bits(res["out"], want), f"{c.id} (flank 0x{poison:02X}): out differs from the ops call"
        got.append(res["out"])
    assert same_bits(got[0], got[1])


@pytest.mark.parametrize("c", APPENDS, ids=[c.id for c in APPENDS])
def test_paged_append_writes_only_q8_and_each_token_s_row(c):
    call, ref = c.make()
    want_q8, written = ref()
    torch.cuda.synchronize()
    assert written
    got = []
    for poison, run, res in _runs(c, call):
        assert same_bits(res["q8"], want_q8), f"{c.id} (flank 0x{poison:02X}): q8 differs from the per-token ops calls"
        for name, idx in (("k_pool", 2), ("v_pool", 3)):
            reg, _, shape = run.outs[name]
            exp = GB.pattern(reg.off, reg.nbytes, _dev()).view(torch.int8).view(shape).clone()
            for w in written:
                exp[w[0], w[1]] = w[idx]
            assert same_bits(res[name], exp), f"{c.id} (flank 0x{poison:02X}): {name} is not its pattern with each token's row written"
        got.append(res)
    for w in written:      # the written bytes do not depend on the flanks (the rest is the arena's pattern, which does)
        for name in ("k_pool", "v_pool"):
            assert same_bits(got[0][name][w[0], w[1]], got[1][name][w[0], w[1]])
    assert same_bits(got[0]["q8"], got[1]["q8"])


@pytest.mark.parametrize("c", NOTHING, ids=[c.id for c in NOTHING])
def test_nothing_to_do_leaves_every_output_byte(c):
    call, _ = c.make()
    for poison, run, _res in _runs(c, call):
        for k, (reg, _, _) in run.outs.items():
            assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), f"{c.id}: an empty call wrote into '{k}'"
