"""Guard bands for the shared-b flag of asq_bmm_i8 (ASQ_BMM_B_GROUP(r) on out_kind: b holds batch / r entries, entry i uses b[i // r]): the raw C-ABI
call, with b placed in a tests/guardband.py arena as the SMALL [batch / r, ...] region it is, returns ASQ_OK, produces the bytes of the ordinary ops
call, leaves every guard and every input as it was, and gives the same output under both input poisons -- a kernel form that still indexed b by the
batch entry would read the flank behind b and fail there.  An empty problem leaves every output byte at its pattern.

One code per kernel form and output width: 0 and 2 ("m16" / "t128"), 18 and 50 ("sm128", full and causal), 130 ("m16kn" / "t128kn").  The cases live
here and not in tests/test_hip_guardband.py's CASES table, as those of tests/test_hip_guardband_bmm_kn.py; the arena plumbing (`Run`) is that file's."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from test_hip_guardband import ASQ_OK, I8, I32, Run, _dev, ri8, same_bits

pytestmark = pytest.mark.gpu

SM, SMC, KN8 = L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX, L.ASQ_BMM_S8 | L.ASQ_BMM_SOFTMAX | L.ASQ_BMM_CAUSAL, L.ASQ_BMM_B_KN | L.ASQ_BMM_S8
CODES = {L.ASQ_BMM_S32: I32, L.ASQ_BMM_S8: I8, SM: I8, SMC: I8, KN8: I8}
SHAPES = [(6, 3, 5, 33, 70), (4, 2, 40, 130, 129)]      # (batch, r, M, N, K): the narrow and the tile kernels, both on the byte path, the latter with 2 column tiles
EMPTY = [(0, 2, 4, 4, 16), (4, 2, 0, 4, 16), (4, 2, 4, 0, 16)]
ALPHA = 2e-4                                            # a score deviation of about 9 for the softmax codes; the int8 codes keep a signal
ARENA_BYTES = 64 << 20

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def ops_call(code, a, b, r):
    if code in (SM, SMC):
        return ops.bmm_i8_softmax_q8(a, b, ALPHA, code == SMC, b_group=r)
    return (ops.bmm_i8_kn if code & L.ASQ_BMM_B_KN else ops.bmm_i8)(a, b, CODES[code], ALPHA, b_group=r)


@pytest.mark.parametrize("skews", [(0, 0), (1, 3)], ids=["aligned", "skewed"])
@pytest.mark.parametrize("code", list(CODES), ids=["s32", "s8", "softmax", "causal", "kn-s8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grouped_kinds_read_only_their_b_and_write_only_their_output(shape, code, skews):
    B, r, M, N, K = shape
    dt, kind = CODES[code], code | L.ASQ_BMM_B_GROUP(r)
    out_skew, in_skew = skews
    out_skew *= torch.empty((), dtype=dt).element_size()       # an output stays aligned to its element
    a, b = ri8((B, M, K), "ga"), ri8((B // r, K, N) if code & L.ASQ_BMM_B_KN else (B // r, N, K), "gb")
    assert L.lib().asq_bmm_kernel_name(B, M, N, K, kind) == L.lib().asq_bmm_kernel_name(B, M, N, K, code) != b"none"
    want = ops_call(code, a, b, r)
    torch.cuda.synchronize()
    assert int(want.abs().max()) > 0
    got = []
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = L.lib().asq_bmm_i8(run.inp("a", a, 16, in_skew), run.inp("b", b, 16, in_skew), run.out("out", (B, M, N), dt, 16, out_skew), kind, B, M, N, K, ALPHA,
                                run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        res = run.results()["out"]
        assert same_bits(res, want), f"flank 0x{poison:02X}: the output differs from the ops call"
        rep = run.arena.check()
        assert rep.ok, f"flank 0x{poison:02X}: {rep}"
        got.append(res)
    assert same_bits(got[0], got[1]), "the output depends on the bytes around the inputs"


@pytest.mark.parametrize("code", list(CODES), ids=["s32", "s8", "softmax", "causal", "kn-s8"])
@pytest.mark.parametrize("shape", EMPTY, ids=["batch0", "M0", "N0"])
def test_nothing_to_do_leaves_every_output_byte(shape, code):
    B, r, M, N, K = shape
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        z = torch.zeros((256,), dtype=I8, device=_dev())
        rc = L.lib().asq_bmm_i8(run.inp("a", z), run.inp("b", z), run.out("out", (256,), torch.uint8, 256), code | L.ASQ_BMM_B_GROUP(r), B, M, N, K, 1.0, run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        reg = run.outs["out"][0]
        assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), "an empty call wrote into 'out'"
        rep = run.arena.check()
        assert rep.ok, str(rep)
