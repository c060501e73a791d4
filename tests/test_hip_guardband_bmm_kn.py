"""Guard bands for the row-major-B kinds of asq_bmm_i8 (out_kind 128, 129, 130 = ASQ_BMM_B_KN | ASQ_BMM_S32 / _F32 / _S8; b is [batch, K, N]): the raw
C-ABI call, with its operands inside a tests/guardband.py arena, returns ASQ_OK, produces the bytes of the ordinary ops.bmm_i8_kn call, leaves
every guard and every input as it was, and gives the same output under both input poisons; an empty problem leaves every output byte at its pattern.

The cases live here and not in tests/test_hip_guardband.py's CASES table (that table is read by the coverage test and by that file's own
parametrisation); the arena plumbing (`Run`) is that file's."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from autosmoothquant_amd import ops
from test_hip_guardband import ASQ_OK, F32, I8, I32, Run, _dev, ri8, same_bits

pytestmark = pytest.mark.gpu

KINDS = {L.ASQ_BMM_B_KN | L.ASQ_BMM_S32: I32, L.ASQ_BMM_B_KN | L.ASQ_BMM_F32: F32, L.ASQ_BMM_B_KN | L.ASQ_BMM_S8: I8}
SHAPES = [(2, 5, 33, 70), (2, 40, 130, 129), (1, 16, 16, 16)]       # m16kn on the byte path, t128kn on the byte path with 2 column tiles, m16kn on the 16-B path
EMPTY = [(0, 4, 4, 16), (2, 0, 4, 16), (2, 4, 0, 16)]
ALPHA = 5e-3
ARENA_BYTES = 64 << 20

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


@pytest.mark.parametrize("skews", [(0, 0), (1, 3)], ids=["aligned", "skewed"])
@pytest.mark.parametrize("kind", list(KINDS), ids=["s32", "f32", "s8"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kn_kinds_write_only_their_output(shape, kind, skews):
    B, M, N, K = shape
    dt = KINDS[kind]
    out_skew, in_skew = skews
    out_skew *= torch.empty((), dtype=dt).element_size()       # an output stays aligned to its element
    a, b = ri8((B, M, K), "kna"), ri8((B, K, N), "knb")
    assert L.lib().asq_bmm_kernel_name(B, M, N, K, kind) == (b"m16kn" if M <= 16 else b"t128kn")
    want = ops.bmm_i8_kn(a, b, dt, ALPHA)
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


@pytest.mark.parametrize("kind", list(KINDS), ids=["s32", "f32", "s8"])
@pytest.mark.parametrize("shape", EMPTY, ids=["batch0", "M0", "N0"])
def test_nothing_to_do_leaves_every_output_byte(shape, kind):
    B, M, N, K = shape
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        z = torch.zeros((256,), dtype=I8, device=_dev())
        rc = L.lib().asq_bmm_i8(run.inp("a", z), run.inp("b", z), run.out("out", (256,), torch.uint8, 256), kind, B, M, N, K, 1.0, run.stream)
        assert rc == ASQ_OK, (rc, L.lib().asq_last_error().decode("utf-8", "replace"))
        torch.cuda.synchronize()
        reg = run.outs["out"][0]
        assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), "an empty call wrote into 'out'"
        rep = run.arena.check()
        assert rep.ok, str(rep)
