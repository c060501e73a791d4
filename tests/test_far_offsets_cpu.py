"""CPU: the case table and the planners of the far-offset tests (tests/far_offsets.py) are what the GPU modules need them to be.

For every case: each far operand has checked bytes below 2^31, in [2^31, 2^32) and at or above 2^32; both wrap models (the offset truncated to 32 bits and read as
unsigned, or sign-extended) send a checked byte of an operand the caller places to another address inside its arena; the stated peak is within 16 GiB.  Every guard
in GUARDS has cases on each side or one of the two accepted reasons.  The shape rules of the pitched cases (the ragged pitch, the special pages, the table and input
pitches) and the device helpers' logic (on small CPU tensors) are checked here too, so that a GPU run does not spend its time on a planner's mistake."""
import pytest
import torch

import far_offsets as F

REASONS = ("exceeds 16 GiB", "unreachable through the C-ABI")


def _checked(f):
    """[lo, hi) byte ranges of the operand's anchor rows"""
    return [(o, o + f.row_bytes) for o in F.far_offsets(f)]


def _hits(ranges, lo, hi):
    return any(a < hi and b > lo for a, b in ranges)


@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_every_far_operand_is_checked_in_all_three_ranges_and_shows_both_wraps(case):
    assert case.far and case.peak <= F.CAP and case.note
    for f in case.far:
        ranges = _checked(f)
        span = F.far_span(f)
        if case.name in F.ENDS_AT_2G:                             # a guard at 2^31: the quantity ends just below it
            assert F.G31 - (1 << 25) < span < F.G31 and not f.apron
            continue
        at_4g = case.name in F.ENDS_AT_4G                         # a guard's own boundary: the operand ends at (or just below) 2^32
        assert span > F.G32 or (at_4g and span > F.G32 - (1 << 20)), f"{case.name}: {f.name} spans {span} bytes"
        assert _hits(ranges, 0, F.G31) and _hits(ranges, F.G31, F.G32) and (at_4g or _hits(ranges, F.G32, span)), f"{case.name}: {f.name} has an unchecked range"
        if not f.apron:
            continue
        lands = {"unsigned": False, "signed": False}
        for a, b in ranges:
            for o in {max(a, F.G31), max(a, F.G32), b - 1}:
                if not a <= o < b:
                    continue
                for model, w in (("unsigned", F.wrap_unsigned(o)), ("signed", F.wrap_signed(o))):
                    if w != o:
                        assert -F.APRON <= w < span, f"{case.name}: {f.name} offset {o} wraps ({model}) to {w}, outside the arena"
                        lands[model] = True
        assert lands["signed"] and (lands["unsigned"] or at_4g), f"{case.name}: {f.name}: {lands}"


def test_case_names_are_distinct_and_every_module_is_named():
    names = [c.name for c in F.CASES]
    assert len(set(names)) == len(names)
    assert {c.module for c in F.CASES} == {"tests.test_hip_far_offsets_kv", "tests.test_hip_far_offsets_rows", "tests.test_hip_far_offsets_gemm", "tests.test_hip_far_offsets_bmm"}


@pytest.mark.parametrize("g", F.GUARDS, ids=[g.name for g in F.GUARDS])
def test_every_guard_has_a_case_on_each_side_or_an_accepted_reason(g):
    names = {c.name for c in F.CASES}
    for side in (g.inside, g.outside):
        if isinstance(side, str):
            assert side.startswith(REASONS), f"{g.name}: '{side}' is not an accepted reason"
        else:
            assert side and set(side) <= names, f"{g.name}: {side}"
    assert g.where


def test_wrap_models():
    assert F.wrap_unsigned(F.G32 + 5) == 5 and F.wrap_unsigned(F.G31 + 5) == F.G31 + 5 and F.wrap_unsigned(7) == 7
    assert F.wrap_signed(F.G31 + 5) == 5 - F.G31 and F.wrap_signed(F.G32 + 5) == 5 and F.wrap_signed(F.G31 - 1) == F.G31 - 1
    assert F.wrap_signed(F.G32 + F.G31) == -F.G31


def test_chunks_cover_without_overlap():
    for rows, step in ((0, 4), (1, 4), (4, 4), (5, 4), (F.ROWS_M16, F.ROWS_CHUNK), (F.ROWS_M32, F.ROWS_CHUNK)):
        c = F.chunks(rows, step)
        assert [a for a, _ in c] == list(range(0, rows, step)) and all(0 < b - a <= step for a, b in c) and (not c or c[-1][1] == rows)
    assert len(F.chunks(F.ROWS_M16, F.ROWS_CHUNK)) == 9 and F.chunks(F.ROWS_M16, F.ROWS_CHUNK)[-1] == (1 << 21, (1 << 21) + 72)


def test_anchor_rows_stand_on_both_sides_of_both_edges():
    for pitch, rows in ((4096, F.ROWS_M16), (8192, F.ROWS_M32), (2048, F.ROWS_M16), (2096, F.pool_pages(2096)), (F.IN_PITCH, 3), (1 << 33, 2)):
        a = F.anchor_rows(pitch, rows)
        assert a == sorted(set(a)) and a[0] == 0 and a[-1] == rows - 1 and len(a) <= 64
        if (rows - 1) * pitch >= F.G32 and pitch < F.G31:
            for edge in (F.G31, F.G32):
                assert any(r * pitch + pitch <= edge for r in a[2:]) and any(edge <= r * pitch < edge + 2 * pitch for r in a), (pitch, rows, edge)


def test_ragged_pitch_puts_sequence_1_on_2g_and_sequence_2_on_4g():
    for s in (F.KV_SMALL, F.KV_R1, F.KV_CHUNKED):
        row, size = s["Hkv"] * s["D"], s["smax"] * s["Hkv"] * s["D"]
        p = F.ragged_pitch(s["smax"], row)
        assert p % 16 == 0 and p % row != 0 and p >= size
        for b, edge in ((1, F.G31), (2, F.G32)):
            first = (edge - b * p) // row                       # the row of sequence b that holds the edge byte
            assert b * p < edge < b * p + size and 2 <= first < s["lengths"][b] - 2, (s, b, first)
        assert max(s["lengths"]) == s["smax"] or s is F.KV_CHUNKED


def test_special_pages_lie_where_their_names_say():
    for pitch in (2048, 2048 + F.POOL_PAD):
        n = F.pool_pages(pitch)
        ids = F.special_pages(pitch, n)
        page = 2048
        assert (n - 1) * pitch >= F.G32 and (n - 4) * pitch < F.G32 + pitch
        for edge in (F.G31, F.G32):
            below = [i for i in ids if i * pitch + page <= edge]
            above = [i for i in ids if i * pitch >= edge]
            assert below and above and edge - (max(below) * pitch + page) < 2 * pitch and min(above) * pitch - edge < pitch
            assert (edge % pitch == 0) or any(i * pitch < edge < i * pitch + pitch for i in ids)
        other = [i + 7 if i + 7 < n else i - 7 for i in ids]
        assert len(set(ids) | set(other) | {1, 3}) == 2 * len(ids) + 2
    assert (2048 + F.POOL_PAD) % 16 == 0 and (2048 + F.POOL_PAD) & (2048 + F.POOL_PAD - 1)


def test_table_and_input_pitches():
    assert F.TABLE_PITCH < F.G31 and F.G31 < F.TABLE_PITCH * 4 < F.G32 < 2 * F.TABLE_PITCH * 4
    assert F.IN_PITCH == F.G31 + 64 and F.IN_PITCH % 16 == 0 and F.G31 <= F.IN_PITCH < F.G32 <= 2 * F.IN_PITCH


def test_fill_and_compare_helpers_on_small_tensors():
    buf = torch.full((1000,), F.FILL, dtype=torch.uint8)
    assert F.is_fill(buf, 0, 1000) and F.is_fill(buf, 3, 997) and F.is_fill(buf, 5, 6)
    for i in (0, 3, 8, 500, 993, 999):
        buf[i] = 0x54
        assert not F.is_fill(buf, 0, 1000), i
        assert F.is_fill(buf, i + 1, 1000) and F.is_fill(buf, 0, i)
        buf[i] = F.FILL
    F.fill_random(buf, 100, 900, 7)
    assert F.is_fill(buf, 0, 100) and F.is_fill(buf, 900, 1000) and not F.is_fill(buf, 100, 900) and F.is_random(buf, 100, 900, 7) and not F.is_random(buf, 100, 900, 8)
    keep = int(buf[333])
    buf[333] = keep ^ 1
    assert not F.is_random(buf, 100, 900, 7) and F.is_random(buf, 100, 900, 7, skip=[(330, 340)]) and not F.is_random(buf, 100, 900, 7, skip=[(334, 340)])


def _names_in_child(env, shapes):
    """ops.gemm_kernel_name for the shapes in a fresh process with `env` (the switches are read once per process); no device is needed"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = f"import sys; sys.path.insert(0, {root!r}); from autosmoothquant_amd import ops; print([ops.gemm_kernel_name(*s) for s in {shapes!r}])"
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    return eval(r.stdout.strip().splitlines()[-1])


def test_dispatcher_decisions_at_the_boundary_one_step_below_and_one_above():
    """the guards whose decision is readable without a device.  The fused forward's N * K < 2^32 is not among them: forward_is_fused is False on both sides (the
    forward does not pick the one-launch kernel at such widths by itself), so tests/test_hip_far_offsets_gemm.py locates it by the explicit entry's own refusal"""
    from autosmoothquant_amd import ops
    top = 1 << 24
    assert [ops.gemm_kernel_name(256, 256, k) == "generic" for k in (top - 128, top, top + 128)] == [False, False, True]
    for kern in F.GEMM_TILED:       # every forced tiled kernel is admitted up to K = 2^24 and not above
        names = _names_in_child({"ASQ_GEMM_KERNEL": kern}, [(256, 256, k) for k in (top - 128, top, top + 128)])
        assert names[0].startswith(kern) and names[1].startswith(kern) and names[2] == "generic", (kern, names)
    k = 1 << 22                     # the forced weight-streaming kernel: M * K < 2^32 at M = 1024
    assert _names_in_child({"ASQ_GEMM_KERNEL": "skinny"}, [(1024, 32, k - 128), (1024, 32, k), (1024, 32, k + 128)]) == ["skinny", "generic", "generic"]
