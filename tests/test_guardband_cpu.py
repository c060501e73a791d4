"""tests/guardband.py on CPU tensors, and the coverage table of the guard-band sweep (tests/test_hip_guardband.py)."""
import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L

# C-ABI entries that write no device memory: pure host-side queries
PURE_QUERIES = {
    "asq_version", "asq_last_error",                                              # a number / the thread-local message
    "asq_offsets_supported", "asq_forward_fused_supported", "asq_gate_up_supported",
    "asq_grouped_gate_up_supported", "asq_fp8_grouped_gate_up_supported",         # *_supported: shape predicates
    "asq_gemm_workspace_bytes", "asq_grouped_workspace_bytes", "asq_linear_w8a8_workspace_bytes",
    "asq_workspace_header_bytes",                                                 # sizes
    "asq_gemm_kernel_name", "asq_bmm_kernel_name",                                # dispatcher introspection
}


def _arena(poison=0x7F):
    return GB.Arena(16 << 20, "cpu", poison)


def test_pattern_depends_on_the_position_and_matches_no_constant_fill():
    p = GB.pattern(0, 1 << 16)
    assert torch.equal(p[4096:8192], GB.pattern(4096, 4096))          # a function of the offset alone
    assert not torch.equal(p[:256], p[256:512])                       # a copied line does not match
    for fill in (0x00, 0x5A, 0x7F, 0xFF):
        assert int((p == fill).sum()) <= p.numel() // 128             # a constant store matches a byte now and then, never a run
        assert int(((p[:-1] == fill) & (p[1:] == fill)).sum()) == 0


@pytest.mark.parametrize("skew", [0, 1, 3, 7])
@pytest.mark.parametrize("align", [1, 2, 16, 256])
def test_place_honours_alignment_skew_and_guard_size(align, skew):
    a = _arena()
    r = a.place(1000, align, skew, "output", "y", pitch=16384)
    assert (r.ptr - skew) % align == 0 and r.ptr == a.base_ptr + r.off
    assert r.off - r.g0 >= GB.guard_bytes(16384) == 128 * 16384 and r.g1 - (r.off + r.nbytes) == 128 * 16384
    assert GB.guard_bytes(0) == GB.guard_bytes(100) == 1 << 20
    assert torch.equal(r.bytes(), GB.pattern(r.off, 1000))            # a not-yet-written output holds the pattern
    assert a.check().ok


@pytest.mark.parametrize("poison", GB.POISONS)
def test_input_flanks_hold_the_poison(poison):
    a = _arena(poison)
    x = torch.arange(64, dtype=torch.float32)
    r = a.place(256, 16, 4, "input", "x", data=x)
    assert torch.equal(r.view(torch.float32, (64,)), x)
    assert bool((a.buf[r.g0:r.off] == poison).all()) and bool((a.buf[r.off + r.nbytes:r.g1] == poison).all())
    assert a.check().ok and a.check().inputs_intact
    if poison == 0xFF:
        assert torch.isnan(a.buf[r.g0:r.g0 + 16].view(torch.float16)).all() and torch.isnan(a.buf[r.g0:r.g0 + 16].view(torch.float32)).all()
    else:
        assert torch.isnan(a.buf[r.g0:r.g0 + 16].view(torch.float16)).all() and float(a.buf[r.g0:r.g0 + 16].view(torch.bfloat16)[0]) > 3e38


@pytest.mark.parametrize("kind", ["output", "workspace", "input"])
@pytest.mark.parametrize("skew", [0, 5])
def test_one_planted_byte_on_either_side_is_found_with_its_offset(skew, kind):
    for side in ("before", "after"):
        a = _arena()
        first = a.place(512, 16, 0, "output", "first")
        r = a.place(777, 16, skew, kind, "victim", data=torch.zeros(777, dtype=torch.uint8) if kind == "input" else None)
        last = a.place(512, 16, 0, "output", "last")
        assert a.check().ok
        at = r.off - 1 if side == "before" else r.off + r.nbytes
        a.buf[at] ^= 0x10
        rep = a.check()
        assert not rep.ok and rep.inputs_intact
        assert rep.guards == [{"region": "victim", "kind": kind, "side": side, "first": at - r.off, "last": at - r.off, "count": 1}], str(rep)
        assert "victim" in str(rep) and side in str(rep)
        assert first.off < r.off < last.off


def test_a_run_of_stray_bytes_reports_first_and_last():
    a = _arena()
    r = a.place(4096, 256, 0, "output", "y", pitch=64)
    a.buf[r.off + 4096:r.off + 4096 + 640] = 0          # ten rows of zeros behind the output
    a.buf[r.off - 64:r.off] = 0x5A
    rep = a.check()
    got = {g["side"]: (g["first"], g["last"]) for g in rep.guards}
    assert got["after"][0] in (4096, 4097) and got["after"][1] in (4096 + 639, 4096 + 638)     # (a pattern byte may itself be 0 at an end)
    assert got["before"][0] in (-64, -63) and got["before"][1] in (-1, -2)


def test_a_changed_input_is_found_and_writes_inside_outputs_are_not():
    a = _arena()
    x = a.place(400, 16, 0, "input", "x", data=torch.ones(100, dtype=torch.float32))
    y = a.place(400, 16, 2, "output", "y")
    w = a.place(4096, 256, 0, "workspace", "ws")
    y.view(torch.float16, (200,)).fill_(3.0)
    w.bytes().zero_()
    assert a.check().ok
    x.view(torch.float32, (100,))[7] = 2.0
    rep = a.check()
    assert not rep.inputs_intact and not rep.guards
    assert [(i["region"], i["first"] // 4, i["last"] // 4) for i in rep.inputs] == [("x", 7, 7)]


def test_reset_reuses_the_arena_and_a_full_arena_refuses():
    a = GB.Arena(3 << 20, "cpu")
    a.place(100, 16, 0, "output", "y")
    with pytest.raises(MemoryError):
        a.place(100, 16, 0, "output", "z")
    a.reset(0xFF)
    r = a.place(100, 16, 0, "input", "x", data=torch.zeros(100, dtype=torch.uint8))
    assert a.poison == 0xFF and int(a.buf[r.off - 1]) == 0xFF and a.check().ok


def test_every_exported_entry_has_a_guard_band_case():
    """a new export without a guard-band case (or without a line in PURE_QUERIES saying why it needs none) fails here"""
    import test_hip_guardband as T
    covered = {c.entry for c in T.CASES}
    assert PURE_QUERIES <= set(L.SIGNATURES), sorted(PURE_QUERIES - set(L.SIGNATURES))
    assert not (covered & PURE_QUERIES)
    assert covered <= set(L.SIGNATURES), sorted(covered - set(L.SIGNATURES))
    missing = sorted(set(L.SIGNATURES) - PURE_QUERIES - covered)
    assert not missing, f"C-ABI entries without a guard-band case in tests/test_hip_guardband.py: {missing}"
    # ... and every writer also has its "nothing to do" case, where the header has one (asq_workspace_init refuses a size below the header)
    empty = {c.entry for c in T.CASES if "-empty-" in c.id}
    assert sorted(covered - empty) == ["asq_workspace_init"]
    for group in [T.CASES] + list(T.FORCED.values()):
        ids = [c.id for c in group]
        assert len(ids) == len(set(ids))
    assert {c[1] for c in T.CHILDREN} - {"gate-up-off"} == set(T.FORCED)
