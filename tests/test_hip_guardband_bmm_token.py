"""Guard bands for the token-major flags of asq_bmm_i8 (ASQ_BMM_A_TOKEN / _B_TOKEN / _OUT_TOKEN with ASQ_BMM_HEADS(h) on out_kind: a flagged operand is
[sequences, rows, heads, cols]): the raw C-ABI call, with every operand placed in a tests/guardband.py arena in the layout its flag states, returns ASQ_OK,
produces the bytes of the ordinary ops call -- so every byte of a token-major out has been written: none still holds the arena's pattern -- leaves every
guard and every input as it was, and gives the same output under both input poisons.  A kernel form that took a dense row pitch or head offset for a
flagged operand, or a token-major one for a dense operand, would read a flank or write a guard here.  An empty problem leaves every output byte.

One code per kernel form and output width: 0 and 2 ("m16" / "t128"), 18 and 50 ("sm128", full and causal), 130 ("m16kn" / "t128kn"), each with every
operand flagged alone and all together (the softmax codes: a, b, both).  The arena plumbing (`Run`) is tests/test_hip_guardband.py's."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from test_hip_guardband import ASQ_OK, I8, I32, Run, _dev, ri8, same_bits

pytestmark = pytest.mark.gpu

SM, SMC, KN8 = L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX, L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX | L.ASQ_BMM_CAUSAL, L.ASQ_BMM_B_KN | L.ASQ_BMM_S8
CODES = {L.ASQ_BMM_S32: I32, L.ASQ_BMM_S8: I8, SM: I8, SMC: I8, KN8: I8}
SHAPES = [(2, 4, 2, 5, 33, 70), (1, 4, 2, 40, 130, 129)]      # (sequences, h, r, M, N, K): the narrow and the tile kernels on the byte path, the latter with 2 column tiles
EMPTY = [(0, 2, 2, 4, 4, 16), (2, 2, 2, 0, 4, 16), (2, 2, 2, 4, 0, 16)]
FLAGGED = [("a", (0, 0)), ("b", (0, 0)), ("o", (0, 0)), ("abo", (1, 3))]      # (flagged operands, (out skew in elements, input skew in bytes))
BITS = {"a": L.ASQ_BMM_A_TOKEN, "b": L.ASQ_BMM_B_TOKEN, "o": L.ASQ_BMM_OUT_TOKEN}
ALPHA = 2e-4                                                  # a score deviation of about 9 for the softmax codes; the int8 codes keep a signal
ARENA_BYTES = 64 << 20

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def ops_call(code, a, b, r, out_token, h):
    heads = {} if a.dim() == 4 else {"heads": h}
    if code in (SM, SMC):
        return ops.bmm_i8_softmax_q8(a, b, ALPHA, code == SMC, b_group=r, **heads)
    return (ops.bmm_i8_kn if code & L.ASQ_BMM_B_KN else ops.bmm_i8)(a, b, CODES[code], ALPHA, b_group=r, out_token=out_token, **heads)


@pytest.mark.parametrize("flagged,skews", FLAGGED, ids=["a", "b", "out", "all-skewed"])
@pytest.mark.parametrize("code", list(CODES), ids=["s32", "s8", "softmax", "causal", "kn-s8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_token_major_kinds_read_only_their_operands_and_write_only_their_output(shape, code, flagged, skews):
    S, h, r, M, N, K = shape
    if code in (SM, SMC):
        flagged = flagged.replace("o", "") or "ab"             # P stays dense: the out case flags both inputs instead
    kn, dt = bool(code & L.ASQ_BMM_B_KN), CODES[code]
    kind = code | L.ASQ_BMM_B_GROUP(r) | L.ASQ_BMM_HEADS(h) | sum(BITS[c] for c in flagged)
    out_skew, in_skew = skews
    out_skew *= torch.empty((), dtype=dt).element_size()       # an output stays aligned to its element
    hb, brows, bcols = h // r, (K if kn else N), (N if kn else K)
    a = ri8((S, M, h, K) if "a" in flagged else (S * h, M, K), "ta", flagged)
    b = ri8((S, brows, hb, bcols) if "b" in flagged else (S * hb, brows, bcols), "tb", flagged)
    out_shape = (S, M, h, N) if "o" in flagged else (S * h, M, N)
    assert L.lib().asq_bmm_kernel_name(S * h, M, N, K, kind) == L.lib().asq_bmm_kernel_name(S * h, M, N, K, code) != b"none"
    want = ops_call(code, a, b, r, "o" in flagged, h)
    torch.cuda.synchronize()
    assert tuple(want.shape) == out_shape and int(want.abs().max()) > 0
    got = []
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = L.lib().asq_bmm_i8(run.inp("a", a, 16, in_skew), run.inp("b", b, 16, in_skew), run.out("out", out_shape, dt, 16, out_skew), kind, S * h, M, N, K, ALPHA,
                                run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        res = run.results()["out"]
        assert same_bits(res, want), f"flank 0x{poison:02X}: the output differs from the ops call (a byte of it may not have been written)"
        rep = run.arena.check()
        assert rep.ok, f"flank 0x{poison:02X}: {rep}"
        got.append(res)
    assert same_bits(got[0], got[1]), "the output depends on the bytes around the inputs"


@pytest.mark.parametrize("code", list(CODES), ids=["s32", "s8", "softmax", "causal", "kn-s8"])
@pytest.mark.parametrize("shape", EMPTY, ids=["batch0", "M0", "N0"])
def test_nothing_to_do_leaves_every_output_byte(shape, code):
    S, h, r, M, N, K = shape
    flags = L.ASQ_BMM_A_TOKEN | L.ASQ_BMM_B_TOKEN | (0 if code in (SM, SMC) else L.ASQ_BMM_OUT_TOKEN)
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        z = torch.zeros((256,), dtype=I8, device=_dev())
        rc = L.lib().asq_bmm_i8(run.inp("a", z), run.inp("b", z), run.out("out", (256,), torch.uint8, 256), code | flags | L.ASQ_BMM_HEADS(h) | L.ASQ_BMM_B_GROUP(r),
                                S * h, M, N, K, 1.0, run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        reg = run.outs["out"][0]
        assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), "an empty call wrote into 'out'"
        rep = run.arena.check()
        assert rep.ok, str(rep)
