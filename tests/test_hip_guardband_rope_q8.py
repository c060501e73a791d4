"""Guard bands for asq_rope_quantize_qkv (include/asq_hip_attn.h): the raw C-ABI call with q, k and v as the three slices of ONE fused [B, S, (Hq + 2 Hkv) D]
input region, q8 a dense output region and k8 / v8 as S-row slots at row `pos` inside cache-sized [B, Smax, Hkv, D] output regions returns ASQ_OK, writes into
q8 and the two slots the bytes of the ordinary ops.rope_quantize_qkv call, leaves every cache byte outside the slots at the arena's pattern, every guard and
every input (the fused buffer and both tables, whole) as they were, and gives the same bytes under both input poisons.  A kernel that took the dense pitch for
a cache, the fused width for an output, or a table row beyond pos + S - 1 would write a pattern byte or read a flank here.  An empty problem (B = 0, S = 0)
leaves every output byte.

CASES is the table tests/test_rope_q8_cpu.py checks against _lib.ATTN_SIGNATURES, with the rule tests/test_guardband_cpu.py keeps for _lib.SIGNATURES; the
arena plumbing (`Run`, `same_bits`, the value generators) is tests/test_hip_guardband.py's."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from test_hip_guardband import ASQ_OK, CODE, FLOATS, I8, NAME, Case, Run, _dev, esize, rnd, same_bits

pytestmark = pytest.mark.gpu

ENTRY = "asq_rope_quantize_qkv"
SCALES = (0.37, 0.11, 0.73)
SHAPES = [(1, 1, 1, 1, 16, 0), (2, 3, 4, 2, 16, 5), (1, 5, 5, 1, 128, 2), (3, 67, 5, 2, 48, 1)]      # (B, S, Hq, Hkv, D, pos): the cache holds pos + S + 3 rows
EMPTY = [("B0", (0, 3, 4, 2, 16)), ("S0", (2, 0, 4, 2, 16))]
ARENA_BYTES = 64 << 20
CASES = []

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def _operands(dt, B, S, Hq, Hkv, D, pos):
    T = pos + S + 2                                             # two table rows behind the last position: they must not be read as data
    fused = rnd(dt, (B, S, (Hq + 2 * Hkv) * D), "q8-qkv", scale=20.0)
    cos, sin = rnd(dt, (T, D // 2), "q8-cos", scale=0.5), rnd(dt, (T, D // 2), "q8-sin", scale=0.5)
    return fused, cos, sin, T


def _full(dt, B, S, Hq, Hkv, D, pos):
    def make():
        from autosmoothquant_amd import ops
        fused, cos, sin, T = _operands(dt, B, S, Hq, Hkv, D, pos)
        ld, smax = (Hq + 2 * Hkv) * D, pos + S + 3
        q, k, v = (fused[..., a * D:b * D].unflatten(-1, (b - a, D)) for a, b in ((0, Hq), (Hq, Hq + Hkv), (Hq + Hkv, Hq + 2 * Hkv)))

        def call(r):
            px, pc, ps = r.inp("qkv", fused), r.inp("cos", cos), r.inp("sin", sin)
            pq8 = r.out("q8", (B, S, Hq, D), I8)
            pk, pv = r.out("k_cache", (B, smax, Hkv * D), I8), r.out("v_cache", (B, smax, Hkv * D), I8)
            slot = pos * Hkv * D
            return L.lib().asq_rope_quantize_qkv(px, px + Hq * D * esize(dt), px + (Hq + Hkv) * D * esize(dt), ld, ld, ld, CODE[dt], pc, ps, T, pos,
                                                 pq8, pk + slot, pv + slot, smax * Hkv * D, *SCALES, B, S, Hq, Hkv, D, r.stream)

        def ref():
            return ops.rope_quantize_qkv(q, k, v, cos, sin, *SCALES, pos=pos)
        return call, ref
    return make


def _empty(dims):
    def make():
        def call(r):
            z = torch.ones((256,), dtype=torch.float16, device=_dev())
            px, pc, ps = r.inp("qkv", z), r.inp("cos", z), r.inp("sin", z)
            outs = [r.out(n, (256,), torch.uint8, 256) for n in ("q8", "k_cache", "v_cache")]
            return L.lib().asq_rope_quantize_qkv(px, px, px, 0, 0, 0, L.ASQ_F16, pc, ps, 8, 0, *outs, 0, *SCALES, *dims, r.stream)
        return call, None
    return make


for _dt in FLOATS:
    for _s in SHAPES:
        CASES.append(Case(ENTRY, f"{ENTRY}-{NAME[_dt]}-B{_s[0]}S{_s[1]}H{_s[2]}+2x{_s[3]}D{_s[4]}-pos{_s[5]}", _full(_dt, *_s)))
for _cid, _dims in EMPTY:
    CASES.append(Case(ENTRY, f"{ENTRY}-empty-{_cid}", _empty(_dims)))
FULL = [c for c in CASES if "-empty-" not in c.id]
NOTHING = [c for c in CASES if "-empty-" in c.id]


def _cache_want(reg, shape, pos, slot):
    """what a cache region must hold after the call: the arena's pattern with rows pos .. pos + S - 1 of every sequence replaced by `slot` [B, S, Hkv, D]"""
    B, smax, row = shape
    want = GB.pattern(reg.off, reg.nbytes, _dev()).view(torch.int8).view(B, smax, row).clone()
    want[:, pos:pos + slot.shape[1]] = slot.reshape(B, slot.shape[1], row)
    return want


@pytest.mark.parametrize("c", FULL, ids=[c.id for c in FULL])
def test_entry_writes_only_q8_and_the_two_cache_slots(c):
    call, ref = c.make()
    q8, k8, v8 = ref()
    torch.cuda.synchronize()
    pos = int(c.id.rsplit("pos", 1)[1])
    assert int(q8.abs().max()) > 0 and int(k8.abs().max()) > 0 and int(v8.abs().max()) > 0
    got = []
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = call(run)
        assert rc == ASQ_OK, (c.id, rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        res = run.results()
        assert same_bits(res["q8"], q8), f"{c.id} (flank 0x{poison:02X}): q8 differs from the ops call"
        for name, slot in (("k_cache", k8), ("v_cache", v8)):
            reg, _, shape = run.outs[name]
            assert same_bits(res[name], _cache_want(reg, shape, pos, slot)), f"{c.id} (flank 0x{poison:02X}): {name} is not its pattern with the slot written"
        rep = run.arena.check()
        assert rep.ok, f"{c.id} (flank 0x{poison:02X}): {rep}"
        got.append(res)
    for name in ("q8", "k_cache", "v_cache"):
        lo, hi = (0, None) if name == "q8" else (pos, pos + k8.shape[1])
        a, b = (got[i][name] if name == "q8" else got[i][name][:, lo:hi] for i in (0, 1))
        assert same_bits(a, b), f"{c.id}: {name} depends on the bytes around the inputs"


@pytest.mark.parametrize("c", NOTHING, ids=[c.id for c in NOTHING])
def test_nothing_to_do_leaves_every_output_byte(c):
    call, _ = c.make()
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = call(run)
        assert rc == ASQ_OK, (c.id, rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        for k, (reg, _, _) in run.outs.items():
            assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), f"{c.id}: an empty call wrote into '{k}'"
        rep = run.arena.check()
        assert rep.ok, f"{c.id}: {rep}"
