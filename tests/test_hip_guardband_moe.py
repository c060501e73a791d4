"""Guard bands for the entries of include/asq_hip_moe.h, with the arena plumbing of tests/test_hip_guardband.py (`Run`, `same_bits`, the value generators), in the
shape of tests/test_hip_guardband_extend.py.

asq_moe_route: logits is an input region; sel, wts, group_offsets, tok and inv are outputs; the scratch is a workspace region of EXACTLY
asq_moe_route_workspace_bytes(T, E, top_k).  asq_moe_dispatch_quantize: x and inv are inputs -- inv with entries below 0 and at or above T * top_k, which a kernel that
trusted them would turn into stores far outside xq --, xq, s_row and row_off outputs.  asq_moe_combine: y, wts and inv (again with entries out of range) are inputs,
out the output.  The raw call returns ASQ_OK, writes the bytes of the ordinary ops call, leaves every guard and every input as it was and gives the same bytes under both
flank poisons.  An empty problem (T == 0) leaves every output byte, except that asq_moe_route writes its all-zero group_offsets.
CASES is the table tests/test_moe_cpu.py checks against _lib.MOE_SIGNATURES."""
import numpy as np
import pytest
import torch

import guardband as GB
import moe_ref as R
from autosmoothquant_amd import _lib as L
from test_hip_guardband import ASQ_OK, CODE, F16, F32, BF16, I8, I32, Case, Run, _dev, rnd, same_bits

pytestmark = pytest.mark.gpu

ROUTE, DISPATCH, COMBINE = "asq_moe_route", "asq_moe_dispatch_quantize", "asq_moe_combine"
ROUTE_SHAPES = [(1, 1, 1, F32), (127, 5, 2, F16), (129, 8, 2, BF16), (389, 64, 8, F16), (7, 8, 8, F32)]                 # (T, E, k, dtype of the logits and the weights)
DISPATCH_SHAPES = [(1, 1, 16, F32, "per-token"), (5, 2, 128, F16, "per-tensor-div"), (70, 2, 4096, BF16, "per-token"), (3, 8, 16384, F16, "per-tensor-round"),
                   (3, 2, 8192, F32, "per-token")]                                                                       # (T, k, K, dtype, mode)
COMBINE_SHAPES = [(1, 1, 8, F16), (37, 2, 4104, BF16), (5, 8, 4096, F32), (300, 2, 4, F32)]                                # (T, k, H, dtype)
MODES = {"per-token": L.ASQ_ACT_PER_TOKEN, "per-tensor-round": L.ASQ_ACT_ROUND, "per-tensor-div": L.ASQ_ACT_DIV}
ARENA_BYTES = 96 << 20
CASES = []

_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def _inv(T, k, key, spoil):
    """a legal inv [T, k] (int32, device); spoil: a few entries far out of range"""
    rng = np.random.default_rng(1000 + T + 7 * k + key)
    inv = rng.permutation(T * k).astype(np.int32).reshape(T, k)
    if spoil:
        flat = inv.reshape(-1)
        for i, v in zip(range(0, T * k, max(1, (T * k) // 3)), (-1, T * k, 1 << 30, -(1 << 31))):
            flat[i] = v
    return torch.from_numpy(inv).to(_dev())


def _route(T, E, k, dt):
    def make():
        from autosmoothquant_amd import ops
        logits = rnd(dt, (T, E), "moe-route", T, E, scale=2.0)
        n = L.lib().asq_moe_route_workspace_bytes(T, E, k)

        def call(r):
            pl = r.inp("logits", logits)
            ps, pw, po = r.out("sel", (T, k), I32), r.out("wts", (T, k), F32), r.out("group_offsets", (E + 1,), I32)
            pt, pi = r.out("tok", (T * k,), I32), r.out("inv", (T, k), I32)
            ws = r.arena.place(n, 16, 0, "workspace", "workspace")
            return L.lib().asq_moe_route(pl, CODE[dt], T, E, k, CODE[dt], ps, pw, po, pt, pi, ws.ptr, n, r.stream)

        def ref():
            return dict(zip(("sel", "wts", "group_offsets", "tok", "inv"), ops.moe_route(logits, k, dt)))
        return call, ref
    return make


def _dispatch(T, k, K, dt, mode):
    def make():
        from autosmoothquant_amd import ops
        x, inv = rnd(dt, (T, K), "moe-disp", T, K), _inv(T, k, K, spoil=T * k >= 4)
        pt = mode == "per-token"

        def call(r):
            px, pi = r.inp("x", x), r.inp("inv", inv)
            pq, po = r.out("xq", (T * k, K), I8), r.out("row_off", (T * k, 2), I32)
            ps = r.out("s_row", (T * k,), F32) if pt else None
            return L.lib().asq_moe_dispatch_quantize(px, CODE[dt], pi, T, k, K, MODES[mode], 0.37, pq, ps, po, r.stream)

        def ref():
            xq, s_row, row_off = ops.moe_dispatch_quantize(x, inv, mode, 0.37, offsets=True)
            return {"xq": xq, "row_off": row_off, **({"s_row": s_row} if pt else {})}
        return call, ref, inv
    return make


def _combine(T, k, H, dt):
    def make():
        from autosmoothquant_amd import ops
        y, inv = rnd(dt, (T * k, H), "moe-comb", T, H), _inv(T, k, H, spoil=T * k >= 4)
        w = torch.rand((T, k), generator=torch.Generator().manual_seed(T + H)).to(_dev())

        def call(r):
            py, pw, pi = r.inp("y", y), r.inp("wts", w), r.inp("inv", inv)
            return L.lib().asq_moe_combine(py, CODE[dt], pw, pi, r.out("out", (T, H), dt), T, k, H, r.stream)

        def ref():
            return {"out": ops.moe_combine(y, w, inv)}
        return call, ref
    return make


def _empty(entry):
    def make():
        def call(r):
            z = torch.ones((256,), dtype=torch.float16, device=_dev())
            px, pn = r.inp("x", z), r.inp("n", torch.zeros((64,), dtype=torch.int32, device=_dev()))
            po, pp = r.out("o0", (256,), torch.uint8, 256), r.out("o1", (256,), torch.uint8, 256)
            if entry == ROUTE:
                return L.lib().asq_moe_route(px, L.ASQ_F16, 0, 8, 2, L.ASQ_F16, po, po, r.out("group_offsets", (9,), I32), pp, pp, None, 0, r.stream)
            if entry == DISPATCH:
                return L.lib().asq_moe_dispatch_quantize(px, L.ASQ_F16, pn, 0, 2, 64, L.ASQ_ACT_PER_TOKEN, 1.0, po, pp, pp, r.stream)
            return L.lib().asq_moe_combine(px, L.ASQ_F16, px, pn, po, 0, 2, 64, r.stream)
        return call, None
    return make


def _name(dt):
    return str(dt)[6:]


for _s in ROUTE_SHAPES:
    CASES.append(Case(ROUTE, f"{ROUTE}-T{_s[0]}E{_s[1]}k{_s[2]}-{_name(_s[3])}", _route(*_s)))
for _s in DISPATCH_SHAPES:
    CASES.append(Case(DISPATCH, f"{DISPATCH}-T{_s[0]}k{_s[1]}K{_s[2]}-{_name(_s[3])}-{_s[4]}", _dispatch(*_s)))
for _s in COMBINE_SHAPES:
    CASES.append(Case(COMBINE, f"{COMBINE}-T{_s[0]}k{_s[1]}H{_s[2]}-{_name(_s[3])}", _combine(*_s)))
for _entry in (ROUTE, DISPATCH, COMBINE):
    CASES.append(Case(_entry, f"{_entry}-empty-T0", _empty(_entry)))
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


@pytest.mark.parametrize("entry", (ROUTE, DISPATCH, COMBINE))
def test_moe_entries_write_only_their_outputs_and_read_no_flank(entry):
    """(one test per entry: every case of WRITERS that calls it)"""
    cases = [c for c in WRITERS if c.entry == entry]
    assert cases
    for c in cases:
        writer_case(c)


def writer_case(c):
    made = c.make()
    call, ref = made[0], made[1]
    want = ref()
    torch.cuda.synchronize()
    written = None
    if c.entry == DISPATCH:                                       # rows no legal inv entry names are not written: they keep the arena's pattern
        inv = made[2].reshape(-1)
        R_ = inv.numel()
        written = torch.zeros((R_,), dtype=torch.bool, device=inv.device)
        written[inv[(inv >= 0) & (inv < R_)].long()] = True
    got = []
    for poison, run, res in _runs(c, call):
        assert set(res) == set(want), (c.id, sorted(res), sorted(want))
        for k, w in want.items():
            have = res[k]
            if written is not None:
                reg = run.outs[k][0]
                pat = GB.pattern(reg.off, reg.nbytes, _dev()).view(have.shape[0], -1)
                assert torch.equal(have.contiguous().view(torch.uint8).view(have.shape[0], -1)[~written], pat[~written]), f"{c.id}: '{k}' has a written row no inv entry names"
                have, w = have[written], w[written]
            assert same_bits(have, w), f"{c.id} (flank 0x{poison:02X}): '{k}' differs from the ops call"
        got.append(res)
    for k in got[0]:
        assert same_bits(got[0][k], got[1][k]), f"{c.id}: output '{k}' depends on the bytes around the inputs"


def test_nothing_to_do_leaves_every_output_byte():
    assert {c.entry for c in NOTHING} == {ROUTE, DISPATCH, COMBINE}
    for c in NOTHING:
        nothing_case(c)


def nothing_case(c):
    call, _ = c.make()
    for poison, run, res in _runs(c, call):
        for k, (reg, _, _) in run.outs.items():
            if k == "group_offsets":
                assert c.entry == ROUTE and res[k].tolist() == [0] * 9, f"{c.id}: group_offsets of an empty routing must be zeros"
            else:
                assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), f"{c.id}: an empty call wrote into '{k}'"
