"""Guard bands for the entries of include/asq_hip_decode.h, with the arena plumbing of tests/test_hip_guardband.py (`Run`, `same_bits`, the value generators).

asq_attn_decode_i8: q, both caches (as [B, max_len + 2 rows] regions: the pitch is wider than max_len rows) and kv_len are input regions, out an output region.  The
raw call returns ASQ_OK, writes the bytes of the ordinary ops.attn_decode_i8 call, leaves every guard and every input as it was and gives the same bytes under both
flank poisons.  kv_len holds entries above max_len and below 0: a kernel that trusted them would read a cache's flank.  The shapes take every ceil(D / 64) of 1 to 4,
the one-pass and the chunked path.
asq_rope_quantize_qkv_at: q, k, v as the three slices of one fused input region, the tables and pos as inputs, q8 and the two whole caches as outputs.  Every cache byte
outside rows pos[b] .. pos[b] + S - 1 of sequence b stays at the arena's pattern, the written rows and q8 equal ops.rope_quantize_qkv called per sequence, and a token
whose position is outside 0 .. min(T, Smax) - 1 writes no cache byte and a zero q8 row.
An empty problem leaves every output byte.  CASES is the table tests/test_attn_decode_cpu.py checks against _lib.DECODE_SIGNATURES."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from test_hip_guardband import ASQ_OK, CODE, FLOATS, I8, NAME, Case, Run, _dev, esize, ri8, rnd, same_bits

pytestmark = pytest.mark.gpu

DECODE, APPEND = "asq_attn_decode_i8", "asq_rope_quantize_qkv_at"
ALPHAS = (0.0009, 1.0 / 127)
SCALES = (0.37, 0.11, 0.73)
# (B, Hq, Hkv, D, max_len, kv_len): the third is chunked (16 rows: 1024 keys per chunk) with a head_dim that is no multiple of 64; the last two are the wide head dims,
# ceil(D / 64) = 3 (r = 3) and 4, the second of them chunked
DECODE_SHAPES = [(2, 4, 2, 64, 40, [49, 17]), (3, 8, 1, 128, 1100, [1100, -3, 1029]), (1, 16, 1, 80, 1300, [1 << 30]), (4, 2, 2, 16, 1, [1, 0, 5, 1]),
                 (2, 6, 2, 192, 70, [70, 33]), (1, 16, 1, 256, 1100, [1100])]
# (B, S, Hq, Hkv, D, Smax, T, pos): positions per sequence; -1, 100 and a slot that crosses min(T, Smax) are out of range in part or in whole
APPEND_SHAPES = [(1, 1, 1, 1, 16, 4, 6, [0]), (3, 1, 8, 2, 128, 9, 12, [8, 0, 5]), (4, 5, 4, 4, 64, 16, 14, [3, -1, 11, 100]), (2, 67, 5, 1, 48, 80, 90, [13, 0])]
ARENA_BYTES = 64 << 20
CASES = []

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def _decode(B, Hq, Hkv, D, ml, kv_len):
    def make():
        from autosmoothquant_amd import ops
        rows = ml + 2
        q, k, v = ri8((B, Hq, D), "dec-q"), ri8((B, rows, Hkv * D), "dec-k"), ri8((B, rows, Hkv * D), "dec-v")
        n = torch.tensor(kv_len, dtype=torch.int32, device=_dev())

        def call(r):
            pq, pk, pv, pn = r.inp("q", q), r.inp("k_cache", k), r.inp("v_cache", v), r.inp("kv_len", n)
            po = r.out("out", (B, Hq, D), I8)
            return L.lib().asq_attn_decode_i8(pq, pk, pv, pn, po, B, Hq, Hkv, D, rows * Hkv * D, ml, *ALPHAS, r.stream)

        def ref():
            return ops.attn_decode_i8(q, k.view(B, rows, Hkv, D)[:, :ml], v.view(B, rows, Hkv, D)[:, :ml], n, *ALPHAS)
        return call, ref
    return make


def _append(dt, B, S, Hq, Hkv, D, smax, T, pos):
    def make():
        from autosmoothquant_amd import ops
        fused = rnd(dt, (B, S, (Hq + 2 * Hkv) * D), "at-qkv", scale=20.0)
        cos, sin = rnd(dt, (T, D // 2), "at-cos", scale=0.5), rnd(dt, (T, D // 2), "at-sin", scale=0.5)
        p = torch.tensor(pos, dtype=torch.int32, device=_dev())
        ld = (Hq + 2 * Hkv) * D
        q, k, v = (fused[..., a * D:b * D].unflatten(-1, (b - a, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))

        def call(r):
            px, pc, ps, pp = r.inp("qkv", fused), r.inp("cos", cos), r.inp("sin", sin), r.inp("pos", p)
            pq8 = r.out("q8", (B, S, Hq, D), I8)
            pk, pv = r.out("k_cache", (B, smax, Hkv * D), I8), r.out("v_cache", (B, smax, Hkv * D), I8)
            return L.lib().asq_rope_quantize_qkv_at(px, px + Hq * D * esize(dt), px + (Hq + Hkv) * D * esize(dt), ld, ld, ld, CODE[dt], pc, ps, T, pp,
                                                    pq8, pk, pv, smax * Hkv * D, smax, *SCALES, B, S, Hq, Hkv, D, r.stream)

        def ref():
            """per sequence: (first row, q8 [S, Hq, D] with zero rows for the skipped tokens, k8 / v8 of the tokens in range) from the single-position op"""
            out = []
            for b in range(B):
                lim = min(T, smax)
                t = 0 if pos[b] < 0 else max(0, min(S, lim - pos[b]))      # tokens 0 .. t - 1 are in range
                q8 = torch.zeros((S, Hq, D), dtype=I8, device=_dev())
                k8 = v8 = torch.zeros((0, Hkv, D), dtype=I8, device=_dev())
                if t:
                    a, k8, v8 = ops.rope_quantize_qkv(q[b:b + 1, :t], k[b:b + 1, :t], v[b:b + 1, :t], cos, sin, *SCALES, pos=pos[b])
                    q8[:t], k8, v8 = a[0], k8[0], v8[0]
                out.append((pos[b], q8, k8, v8))
            return out
        return call, ref
    return make


def _empty(entry, dims):
    def make():
        def call(r):
            z = torch.ones((256,), dtype=torch.float16, device=_dev())
            px, pn = r.inp("x", z), r.inp("n", torch.zeros((64,), dtype=torch.int32, device=_dev()))
            outs = [r.out(n, (256,), torch.uint8, 256) for n in ("o0", "o1", "o2")]
            if entry == DECODE:
                return L.lib().asq_attn_decode_i8(px, px, px, pn, outs[0], *dims, 0, 8, *ALPHAS, r.stream)
            return L.lib().asq_rope_quantize_qkv_at(px, px, px, 0, 0, 0, L.ASQ_F16, px, px, 8, pn, *outs, 0, 8, *SCALES, *dims, r.stream)
        return call, None
    return make


for _s in DECODE_SHAPES:
    CASES.append(Case(DECODE, f"{DECODE}-B{_s[0]}H{_s[1]}x{_s[2]}D{_s[3]}-max{_s[4]}", _decode(*_s)))
for _dt in FLOATS:
    for _s in APPEND_SHAPES:
        CASES.append(Case(APPEND, f"{APPEND}-{NAME[_dt]}-B{_s[0]}S{_s[1]}H{_s[2]}+2x{_s[3]}D{_s[4]}-rows{_s[5]}", _append(_dt, *_s)))
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
def test_decode_writes_only_out_and_reads_no_flank(c):
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
def test_append_writes_only_q8_and_each_sequence_s_rows(c):
    call, ref = c.make()
    want = ref()
    torch.cuda.synchronize()
    got = []
    for poison, run, res in _runs(c, call):
        assert same_bits(res["q8"], torch.stack([w[1] for w in want])), f"{c.id} (flank 0x{poison:02X}): q8 differs from the per-sequence ops calls"
        for name, idx in (("k_cache", 2), ("v_cache", 3)):
            reg, _, shape = run.outs[name]
            exp = GB.pattern(reg.off, reg.nbytes, _dev()).view(torch.int8).view(shape).clone()
            for b, w in enumerate(want):
                if w[idx].shape[0]:
                    exp[b, w[0]:w[0] + w[idx].shape[0]] = w[idx].reshape(w[idx].shape[0], shape[2])
            assert same_bits(res[name], exp), f"{c.id} (flank 0x{poison:02X}): {name} is not its pattern with each sequence's rows written"
        got.append(res)
    for b, w in enumerate(want):      # the written bytes do not depend on the flanks (the rest is the arena's pattern, which does)
        for name, idx in (("k_cache", 2), ("v_cache", 3)):
            rows = slice(w[0], w[0] + w[idx].shape[0])
            assert same_bits(got[0][name][b, rows], got[1][name][b, rows])
    assert same_bits(got[0]["q8"], got[1]["q8"])


@pytest.mark.parametrize("c", NOTHING, ids=[c.id for c in NOTHING])
def test_nothing_to_do_leaves_every_output_byte(c):
    call, _ = c.make()
    for poison, run, _res in _runs(c, call):
        for k, (reg, _, _) in run.outs.items():
            assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), f"{c.id}: an empty call wrote into '{k}'"
