"""Guard-band sweep: every C-ABI entry that writes device memory writes only its own outputs, and reads nothing that counts from
beyond its inputs.

Each case runs one raw C-ABI call (pointers into a tests/guardband.py arena, the current stream) and checks
  1. the return code is ASQ_OK;
  2. every output region equals, bit for bit, what the ordinary ops.* call returns for the same operands in ordinary tensors
     (every comparison here is equality, between two launches of the same kernel: what ties those calls to the oracle is the rest of the suite -- at the
     ladder lengths of this file tests/test_hip_row_ladders.py, at model sizes the test_hip_* file of each family);
  3. every guard is intact -- also the one behind a workspace of exactly asq_*_workspace_bytes(...) bytes;
  4. every input region (for a strided input: the whole buffer, the bytes between its rows included) is unchanged;
  5. the outputs are identical under the 0x7F and the 0xFF input flanks.

CASES is a flat table of (entry, id, factory); tests/test_guardband_cpu.py checks that it names every symbol of _lib.SIGNATURES that
writes device memory.  The table is built without touching the device, operands are made when a case runs.

Dispatch tiers that no public call reaches (recorded here instead of inventing a case):
  * quant_per_token_cached<NV = 1, 2, 4, 6> (asq_quantize_act, per-token): the wave-per-row kernel takes every K / VEC <= 1792, so the
    block-per-row ladder starts at NV = 8; a row that fails the vector checks (K % VEC, alignment) goes to quant_per_token_generic.
  * quant_rows_off<NV = 1, 2, 4> (asq_quantize_act_off): the wave kernel takes K / VEC <= 1536 (per-token: 1792), the entry refuses
    unaligned rows, so only NV = 8 and 20 run; quant_rows_wave<28> exists for per-token rows only.
  * fp8_quant_per_token with vec = 1 at K / VEC <= 1792: taken by fp8_quant_rows_wave; it runs above that and, with vec = 0, on rows that
    fail the vector checks (ASQ_FP8_ROWS_WAVE=0 is an A/B switch, not a dispatch path).
  * the tiled GEMM kernels need K % 128 == 0 and 16-byte aligned operands: "K one below / above a tile" exists for the generic kernel only;
    the tiled ones get K at 1 and at 2 or 3 tiles.  asq_linear_w8a8_gate_up[_q8] need M % 256 == 0, F % 128 == 0, K % 256 == 0: F varies by
    half a tile, M and K by whole ones.
  * the weight-streaming kernel's in-launch reduction (a workspace for "skinny") starts at weights of ~100 MB (32 x 5120 x 20480): left to
    test_hip_parity.py; the workspace guard is checked on the K split of the 128 x 128 kernel and on the grouped launches instead."""
import os
import subprocess
import sys
import zlib
from collections import namedtuple

import pytest
import torch

import guardband as GB
from autosmoothquant_amd import _lib as L
from row_ladders import NORM, OFF_BLOCK, PT_BLOCK, SILU, WAVE_F8, WAVE_I8, ladder

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
I8, I32, U8 = torch.int8, torch.int32, torch.uint8
FLOATS = (F32, F16, BF16)
CODE = {F32: L.ASQ_F32, F16: L.ASQ_F16, BF16: L.ASQ_BF16}
VEC = {F32: 4, F16: 8, BF16: 8}
NAME = {F32: "f32", F16: "f16", BF16: "bf16", I8: "i8", I32: "i32", U8: "u8"}
ROWS = (1, 2, 3, 4, 5, 4099)          # M of the row kernels: below / at / above the 4 rows of a wave-per-row block, and one M above 4096
ASQ_OK, ASQ_ERR_DIM = 0, -2              # include/asq_hip.h status codes
ARENA_BYTES = 600 << 20               # one arena for the whole file (the grouped workspace alone is 64 MiB + a header)

Case = namedtuple("Case", "entry id make")   # make() -> (call(run) -> rc, ref() -> {output name: tensor})
CASES = []
FORCED = {}                                  # child-process groups: name -> [Case]


def case(entry, cid, group=None):
    def deco(make):
        (CASES if group is None else FORCED.setdefault(group, [])).append(Case(entry, f"{entry}-{cid}", make))
        return make
    return deco


def _dev():
    return torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def rnd(dt, shape, *key, scale=3.0):
    """normal values (a few of them large) of dtype dt on the device"""
    t = torch.randn(shape, generator=_gen("rnd", dt, shape, key)) * scale
    if t.numel():
        t.view(-1)[:: max(1, t.numel() // 7)] *= 17.0
    return t.to(dt).to(_dev())


def ri8(shape, *key):
    return torch.randint(-128, 128, shape, generator=_gen("i8", shape, key), dtype=I8).to(_dev())


def rpos(shape, *key, scale=1e-2):
    return (torch.rand(shape, generator=_gen("pos", shape, key)) * scale + 1e-3).to(_dev())


def rf8(shape, *key):
    return (torch.randn(shape, generator=_gen("f8", shape, key)) * 2).to(_dev()).to(torch.float8_e4m3fn)


def esize(dt):
    return torch.empty((), dtype=dt).element_size()


class Run:
    """One raw call's operands inside the arena."""

    def __init__(self, arena, poison):
        arena.reset(poison)
        self.arena, self.outs = arena, {}
        self.stream = _stream()

    def inp(self, name, t, align=16, skew=0):
        if t is None:
            return None
        pitch = t.shape[-1] * t.element_size() if t.dim() >= 2 else 0        # (a flat operand has no rows)
        return self.arena.place(t.numel() * t.element_size(), align, skew, "input", name, pitch, data=t).ptr

    def out(self, name, shape, dt, align=16, skew=0, init=None):
        n = 1
        for s in shape:
            n *= s
        pitch = shape[-1] * esize(dt) if len(shape) >= 2 else 0
        r = self.arena.place(n * esize(dt), align, skew, "output", name, pitch, data=init)
        self.outs[name] = (r, dt, tuple(shape))
        return r.ptr

    def ws(self, nbytes):
        """a workspace of EXACTLY nbytes, 256-byte aligned, initialised once as the header asks"""
        if nbytes == 0:
            return None, 0
        assert nbytes > L.lib().asq_workspace_header_bytes() or not os.environ.get("ASQ_KSPLIT"), "a forced K split needs scratch"
        r = self.arena.place(nbytes, 256, 0, "workspace", "workspace")
        L.check(L.lib().asq_workspace_init(r.ptr, nbytes, self.stream), "asq_workspace_init")
        return r.ptr, nbytes

    def results(self):
        return {k: r.view(dt, shape).clone() for k, (r, dt, shape) in self.outs.items()}


_arena = None


def arena():
    global _arena
    if _arena is None:
        _arena = GB.Arena(ARENA_BYTES, _dev())
    return _arena


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(-1).view(U8), b.contiguous().view(-1).view(U8))


def run_case(c):
    call, ref = c.make()
    want = {k: v for k, v in ref().items() if v is not None}
    torch.cuda.synchronize()
    got = []
    for poison in GB.POISONS:
        run = Run(arena(), poison)
        rc = call(run)
        assert rc == ASQ_OK, (c.id, rc, L.lib().asq_last_error().decode("utf-8", "replace"))           # 1
        torch.cuda.synchronize()
        res = run.results()
        assert set(res) == set(want), (c.id, sorted(res), sorted(want))
        for k, w in want.items():                                                                          # 2
            if w.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
                w = w.view(U8)
            have = res[k] if w.numel() == res[k].numel() else res[k].reshape(-1)[:w.numel()]     # (a declared scratch tail: see _quantize_act_fp8)
            w = w.reshape(have.shape)
            if not same_bits(have, w):
                bad = torch.nonzero(have.reshape(-1).view(U8) != w.contiguous().reshape(-1).view(U8)).reshape(-1)
                raise AssertionError(f"{c.id}: output '{k}' differs from the ops.* result under flank 0x{poison:02X}: {bad.numel()} bytes, first at {int(bad[0])}, last at {int(bad[-1])}")
        rep = run.arena.check()                                                                            # 3, 4
        assert rep.ok, f"{c.id} (flank 0x{poison:02X}): {rep}"
        got.append(res)
    for k in got[0]:                                                                                       # 5
        assert same_bits(got[0][k], got[1][k]), f"{c.id}: output '{k}' depends on the bytes around the inputs"


# =====================================================================================================================================
# K ladders of the row kernels (asq_quant.hip / asq_fp8.hip): per tier its top, the first K of the next tier, a partial last 64-lane round
# =====================================================================================================================================
# (the tier tuples and ladder() live in tests/row_ladders.py, shared with tests/test_hip_row_ladders.py; tests/test_row_ladders_cpu.py ties them to the sources)


def rows_for(i):
    return ROWS[i % 5]


# ---- asq_quantize_act / _off ----------------------------------------------------------------------------------------------------------
_MODES = {"per-token": L.ASQ_ACT_PER_TOKEN, "per-tensor-round": L.ASQ_ACT_ROUND, "per-tensor-div": L.ASQ_ACT_DIV}


def _quantize_act(dt, mode, M, K, xq_skew=0, x_skew=0, off=False):
    def make():
        from autosmoothquant_amd import ops
        x = rnd(dt, (M, K), "qa", mode)
        pt = mode == "per-token"

        def call(r):
            px = r.inp("x", x, 16, x_skew)
            pq = r.out("xq", (M, K), I8, 16, xq_skew)
            ps = r.out("s_row", (M,), F32, 16, 4) if pt else None
            if off:
                po = r.out("row_off", (M, 2), I32, 16, 8)
                return L.lib().asq_quantize_act_off(px, CODE[dt], _MODES[mode], 0.37, pq, ps, po, M, K, r.stream)
            return L.lib().asq_quantize_act(px, CODE[dt], _MODES[mode], 0.37, pq, ps, M, K, r.stream)

        def ref():
            if off:
                q, s, o = ops.quantize_act_off(x, mode, 0.37)
                return {"xq": q, "s_row": s, "row_off": o}
            q, s = ops.quantize_act(x, mode, 0.37)
            return {"xq": q, "s_row": s}
        return call, ref
    return make


for dt in FLOATS:
    v = VEC[dt]
    # per-token: the wave ladder, then quant_per_token_cached<8, 12, 20>, then the generic kernel (K / VEC > 5120)
    ks = ladder(WAVE_I8, 64, 1793) + ladder(PT_BLOCK, 256, 5121, lo=1793)
    for i, nvec in enumerate(ks):
        case("asq_quantize_act", f"pt-{NAME[dt]}-nvec{nvec}")(_quantize_act(dt, "per-token", rows_for(i), nvec * v, xq_skew=v))
    for M in ROWS:
        case("asq_quantize_act", f"pt-{NAME[dt]}-M{M}")(_quantize_act(dt, "per-token", M, 27 * v, xq_skew=v))
    # generic rows: K not a multiple of VEC; x at element alignment; xq at byte alignment
    case("asq_quantize_act", f"pt-{NAME[dt]}-generic-K")(_quantize_act(dt, "per-token", 5, 64 * v + 3, xq_skew=0))
    case("asq_quantize_act", f"pt-{NAME[dt]}-generic-x")(_quantize_act(dt, "per-token", 3, 64 * v, x_skew=esize(dt)))
    case("asq_quantize_act", f"pt-{NAME[dt]}-generic-xq")(_quantize_act(dt, "per-token", 4, 65 * v, xq_skew=1))
    # the per-tensor modes are flat: 16-element chunks + a scalar remainder (none / only / both), scalar only when a pointer is unaligned
    for mode in ("per-tensor-round", "per-tensor-div"):
        for (M, K) in ((1, 16), (1, 15), (3, 37), (5, 256 * 16 + 16), (5, 4099), (4099, 16), (4099, 5), (4099, 4100)):      # (the last: more chunks than the capped grid of 4096 blocks carries in one sweep)
            case("asq_quantize_act", f"{mode}-{NAME[dt]}-{M}x{K}")(_quantize_act(dt, mode, M, K))
        case("asq_quantize_act", f"{mode}-{NAME[dt]}-unaligned-xq")(_quantize_act(dt, mode, 3, 48, xq_skew=1))
        case("asq_quantize_act", f"{mode}-{NAME[dt]}-unaligned-x")(_quantize_act(dt, mode, 3, 48, x_skew=esize(dt)))
    # offset images: wave ladder (per-tensor rows: up to 24 vectors per lane, per-token 28), then quant_rows_off<8, 20>
    for mode, top in (("per-token", 1792), ("per-tensor-round", 1536)):
        ks = ladder(WAVE_I8, 64, top + 1) + ladder(OFF_BLOCK, 256, 5120, lo=top + 1)
        for i, nvec in enumerate(ks):
            case("asq_quantize_act_off", f"{mode}-{NAME[dt]}-nvec{nvec}")(_quantize_act(dt, mode, rows_for(i + 2), nvec * v, xq_skew=v, off=True))
    for nvec in (27, 64, 1536, 1537, 2049, 5120):
        case("asq_quantize_act_off", f"per-tensor-div-{NAME[dt]}-nvec{nvec}")(_quantize_act(dt, "per-tensor-div", 5, nvec * v, xq_skew=v, off=True))
    for M in ROWS:
        case("asq_quantize_act_off", f"pt-{NAME[dt]}-M{M}")(_quantize_act(dt, "per-token", M, 65 * v, xq_skew=v, off=True))


# ---- the norm -> int8 family (norm_quant_cached<NV = 1, 2, 4, 8>: one block per row, K / VEC <= 2048) -------------------------------------
NORM_KS = ladder(NORM, 256, 2048)


def _norm_quantize(entry, dt, M, K, ln, pt, inplace=False, xq_skew=None):
    """entry: asq_norm_quantize | asq_norm_quantize_off | asq_add_norm_quantize | asq_add_norm_quantize_off"""
    off, add = entry.endswith("_off"), "add_norm" in entry

    def make():
        from autosmoothquant_amd import ops
        x, res = rnd(dt, (M, K), "nq", entry), rnd(dt, (M, K), "nq-res", entry)
        w, b = rnd(dt, (K,), "nq-w", scale=1.0), (rnd(dt, (K,), "nq-b", scale=1.0) if ln else None)

        def call(r):
            px = None if inplace == "x" else r.inp("x", x)
            if add:       # include/asq_hip.h: "h_out may alias residual or x"
                ph = r.out("h", (M, K), dt, init={True: res, "x": x}.get(inplace))
                pr = ph if inplace is True else r.inp("residual", res)
                px = ph if inplace == "x" else px
            pw, pb = r.inp("weight", w), r.inp("bias", b)
            pq = r.out("xq", (M, K), I8, 16, VEC[dt] if xq_skew is None else xq_skew)
            ps = r.out("s_row", (M,), F32, 16, 4) if pt else None
            po = r.out("row_off", (M, 2), I32, 16, 8) if off else None
            lib = L.lib()
            if entry == "asq_norm_quantize":
                return lib.asq_norm_quantize(px, CODE[dt], pw, pb, 1e-5, int(pt), pq, ps, M, K, r.stream)
            if entry == "asq_norm_quantize_off":
                return lib.asq_norm_quantize_off(px, CODE[dt], pw, pb, 1e-5, int(pt), pq, ps, po, M, K, r.stream)
            if entry == "asq_add_norm_quantize":
                return lib.asq_add_norm_quantize(px, pr, ph, CODE[dt], pw, pb, 1e-5, int(pt), pq, ps, M, K, r.stream)
            return lib.asq_add_norm_quantize_off(px, pr, ph, CODE[dt], pw, pb, 1e-5, int(pt), pq, ps, po, M, K, r.stream)

        def ref():
            if add:
                t = ops.add_norm_quantize(x, res, w, b, 1e-5, pt, offsets=off)
                return dict(zip(("h", "xq", "s_row", "row_off"), t))
            return dict(zip(("xq", "s_row", "row_off"), ops.norm_quantize(x, w, b, 1e-5, pt, offsets=off)))
        return call, ref
    return make


for entry in ("asq_norm_quantize", "asq_norm_quantize_off", "asq_add_norm_quantize", "asq_add_norm_quantize_off"):
    for dt in FLOATS:
        for i, nvec in enumerate(NORM_KS):
            ln, pt = bool(i & 1), bool(i & 2)
            case(entry, f"{NAME[dt]}-nvec{nvec}-{'ln' if ln else 'rms'}-{'pt' if pt else 'tensor'}")(_norm_quantize(entry, dt, rows_for(i), nvec * VEC[dt], ln, pt))
        for ln in (False, True):
            for pt in (False, True):
                case(entry, f"{NAME[dt]}-variants-{'ln' if ln else 'rms'}-{'pt' if pt else 'tensor'}")(_norm_quantize(entry, dt, 3, 91 * VEC[dt], ln, pt))
        for M in ROWS:
            case(entry, f"{NAME[dt]}-M{M}")(_norm_quantize(entry, dt, M, 27 * VEC[dt], M & 1 == 0, M & 2 == 0))
        if "add_norm" in entry:   # the residual stream updated in place: h_out == residual
            for i, nvec in enumerate((91, 256, 257, 2048)):
                case(entry, f"{NAME[dt]}-inplace-nvec{nvec}")(_norm_quantize(entry, dt, rows_for(i + 1), nvec * VEC[dt], bool(i & 1), not (i & 2), inplace=True))
                case(entry, f"{NAME[dt]}-h-is-x-nvec{nvec}")(_norm_quantize(entry, dt, rows_for(i + 2), nvec * VEC[dt], not (i & 1), bool(i & 2), inplace="x"))


def _dq_add_layernorm_q(dt, M, K, inplace):
    def make():
        from autosmoothquant_amd import ops
        x = torch.randint(-200000, 200000, (M, K), generator=_gen("dq", M, K), dtype=I32).to(_dev())
        res, g, b = rnd(dt, (M, K), "dq-res"), rnd(dt, (K,), "dq-g", scale=1.0), rnd(dt, (K,), "dq-b", scale=1.0)

        def call(r):
            px = r.inp("x", x)
            ph = r.out("h", (M, K), dt, init=res) if inplace else r.out("h", (M, K), dt)
            pr = ph if inplace else r.inp("residual", res)
            pq = r.out("q", (M, K), I8, 16, VEC[dt])
            return L.lib().asq_dq_add_layernorm_q(px, 3.1e-4, pr, ph, CODE[dt], r.inp("gamma", g), r.inp("beta", b), 1e-5, pq, M, K, r.stream)

        def ref():
            return dict(zip(("h", "q"), ops.dq_add_layernorm_q(x, 3.1e-4, res, g, b, 1e-5)))
        return call, ref
    return make


for dt in FLOATS:
    for i, nvec in enumerate(NORM_KS):
        case("asq_dq_add_layernorm_q", f"{NAME[dt]}-nvec{nvec}{'-inplace' if i % 3 == 0 else ''}")(_dq_add_layernorm_q(dt, rows_for(i), nvec * VEC[dt], i % 3 == 0))
    for M in ROWS:
        case("asq_dq_add_layernorm_q", f"{NAME[dt]}-M{M}")(_dq_add_layernorm_q(dt, M, 27 * VEC[dt], M & 1 == 1))


def _rmsnorm(dt, M, K):
    def make():
        from autosmoothquant_amd import ops
        x, w = rnd(dt, (M, K), "rms"), rnd(dt, (K,), "rms-w", scale=1.0)

        def call(r):
            return L.lib().asq_rmsnorm(r.inp("x", x), CODE[dt], r.inp("weight", w), 1e-5, r.out("y", (M, K), dt), M, K, r.stream)
        return call, lambda: {"y": ops.rmsnorm(x, w, 1e-5)}
    return make


for dt in FLOATS:
    for i, nvec in enumerate(NORM_KS):
        case("asq_rmsnorm", f"{NAME[dt]}-nvec{nvec}")(_rmsnorm(dt, rows_for(i), nvec * VEC[dt]))
    for M in ROWS:
        case("asq_rmsnorm", f"{NAME[dt]}-M{M}")(_rmsnorm(dt, M, 27 * VEC[dt]))


# ---- SiLU(gate) * up: int8 (silu_mul_quant_cached<2, 4, 6, 8>), e4m3 (silu_mul_quant_fp8_cached<2, 4, 6, 8>), floating (flat) --------------
SILU_KS = ladder(SILU, 256, 2048)


def _silu_mul_quantize(entry, dt, M, K, pt, fast):
    off, f8 = entry.endswith("_off"), entry.endswith("_fp8")

    def make():
        from autosmoothquant_amd import ops
        g, u = rnd(dt, (M, K), "sm-g", entry), rnd(dt, (M, K), "sm-u", entry, scale=2.0)

        def call(r):
            pg, pu = r.inp("gate", g), r.inp("up", u)
            lib = L.lib()
            if f8:
                pq, ps = r.out("xq", (M, K), U8, 16, 8), r.out("scale", (M,), F32, 16, 4)
                return lib.asq_silu_mul_quantize_fp8(pg, pu, CODE[dt], 2 if fast else 0, pq, ps, M, K, r.stream)
            pq = r.out("xq", (M, K), I8, 16, VEC[dt])
            ps = r.out("s_row", (M,), F32, 16, 4) if pt else None
            flags = (1 if pt else 0) | (2 if fast else 0)
            if off:
                return lib.asq_silu_mul_quantize_off(pg, pu, CODE[dt], flags, 0.21, pq, ps, r.out("row_off", (M, 2), I32, 16, 8), M, K, r.stream)
            return lib.asq_silu_mul_quantize(pg, pu, CODE[dt], flags, 0.21, pq, ps, M, K, r.stream)

        def ref():
            if f8:
                return dict(zip(("xq", "scale"), ops.silu_mul_quantize_fp8(g, u, fast)))
            return dict(zip(("xq", "s_row", "row_off"), ops.silu_mul_quantize(g, u, pt, 0.21, fast, offsets=off)))
        return call, ref
    return make


for entry in ("asq_silu_mul_quantize", "asq_silu_mul_quantize_off", "asq_silu_mul_quantize_fp8"):
    for dt in FLOATS:
        for i, nvec in enumerate(SILU_KS):
            pt, fast = bool(i & 1), bool(i & 2)
            case(entry, f"{NAME[dt]}-nvec{nvec}-{'pt' if pt else 'tensor'}{'-fast' if fast else ''}")(_silu_mul_quantize(entry, dt, rows_for(i), nvec * VEC[dt], pt, fast))
        for pt in (False, True):
            for fast in (False, True):
                case(entry, f"{NAME[dt]}-variants-{'pt' if pt else 'tensor'}{'-fast' if fast else ''}")(_silu_mul_quantize(entry, dt, 3, 91 * VEC[dt], pt, fast))
        for M in ROWS:
            case(entry, f"{NAME[dt]}-M{M}")(_silu_mul_quantize(entry, dt, M, 27 * VEC[dt], M & 1 == 1, M & 2 == 2))


def _silu_mul(dt, n, fast):
    def make():
        from autosmoothquant_amd import ops
        g, u = rnd(dt, (n,), "smf-g"), rnd(dt, (n,), "smf-u")

        def call(r):
            return L.lib().asq_silu_mul(r.inp("gate", g), r.inp("up", u), CODE[dt], 2 if fast else 0, r.out("out", (n,), dt), n, r.stream)
        return call, lambda: {"out": ops.silu_mul(g, u, fast)}
    return make


for dt in FLOATS:
    # one vector; a partial block; one block + one vector; more vectors than the grid's 256 * 64 blocks of 256 threads carry in one sweep
    for i, nvec in enumerate((1, 27, 256, 257, 256 * 64 * 256 + 91)):
        case("asq_silu_mul", f"{NAME[dt]}-nvec{nvec}")(_silu_mul(dt, nvec * VEC[dt], bool(i & 1)))


# ---- fp8 quantisers -------------------------------------------------------------------------------------------------------------------------
_F8MODES = {"per-token": L.ASQ_FP8_PER_TOKEN, "per-tensor": L.ASQ_FP8_PER_TENSOR, "static": L.ASQ_FP8_STATIC}


def _quantize_act_fp8(dt, mode, M, K, x_skew=0, xq_skew=8):
    def make():
        from autosmoothquant_amd import ops
        x = rnd(dt, (M, K), "qf8", mode)

        def call(r):
            px, pq = r.inp("x", x, 16, x_skew), r.out("xq", (M, K), U8, 16, xq_skew)
            ps = r.out("scale", (M,) if mode == "per-token" else (2,), F32, 16, 4) if mode != "static" else None
            return L.lib().asq_quantize_act_fp8(px, CODE[dt], _F8MODES[mode], 0.043, pq, ps, M, K, r.stream)

        def ref():
            q, s = ops.quantize_act_fp8(x, mode, 0.043)
            if mode == "per-token":
                return {"xq": q, "scale": s.reshape(M)}
            if mode == "per-tensor":                  # include/asq_hip.h: "scale_out f32[2]: [0] receives the scale, [1] is scratch" -- [0] is compared with ops,
                return {"xq": q, "scale": s.reshape(1)}   # [1] only between the two flank runs (run_case: a shorter reference compares the prefix)
            return {"xq": q}
        return call, ref
    return make


for dt in FLOATS:
    v = VEC[dt]
    for i, nvec in enumerate(ladder(WAVE_F8, 64, 1793)):     # 1793: the first row length of the block-per-row kernel
        case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-nvec{nvec}")(_quantize_act_fp8(dt, "per-token", rows_for(i), nvec * v))
    for M in ROWS:
        case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-M{M}")(_quantize_act_fp8(dt, "per-token", M, 27 * v))
    case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-block-long")(_quantize_act_fp8(dt, "per-token", 3, 2048 * v + v))
    case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-scalar-K")(_quantize_act_fp8(dt, "per-token", 5, 64 * v + 3))
    case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-scalar-x")(_quantize_act_fp8(dt, "per-token", 3, 64 * v, x_skew=esize(dt)))
    case("asq_quantize_act_fp8", f"pt-{NAME[dt]}-scalar-xq")(_quantize_act_fp8(dt, "per-token", 4, 65 * v, xq_skew=1))
    for mode in ("per-tensor", "static"):
        for (M, K) in ((1, 8), (1, 7), (3, 37), (5, 256 * 8 + 8), (4099, 8), (4099, 5), (4099, 2056)):     # (the last: more than the capped grid of 4096 blocks carries in one sweep)
            case("asq_quantize_act_fp8", f"{mode}-{NAME[dt]}-{M}x{K}")(_quantize_act_fp8(dt, mode, M, K))
        case("asq_quantize_act_fp8", f"{mode}-{NAME[dt]}-unaligned-xq")(_quantize_act_fp8(dt, mode, 3, 48, xq_skew=1))
        case("asq_quantize_act_fp8", f"{mode}-{NAME[dt]}-unaligned-x")(_quantize_act_fp8(dt, mode, 3, 48, x_skew=esize(dt)))


def _cast_e5m2(dt, M, K, x_skew=0, xq_skew=0):
    def make():
        from autosmoothquant_amd import ops
        x = rnd(dt, (M, K), "e5m2", scale=300.0)

        def call(r):
            return L.lib().asq_cast_e5m2(r.inp("x", x, 16, x_skew), CODE[dt], r.out("xq", (M, K), U8, 16, xq_skew), M * K, r.stream)
        return call, lambda: {"xq": ops.cast_e5m2(x)}
    return make


for dt in FLOATS:
    for (M, K) in ((1, 8), (1, 7), (3, 37), (5, 256 * 8 + 8), (4099, 8), (4099, 5), (4099, 2056)):
        case("asq_cast_e5m2", f"{NAME[dt]}-{M}x{K}")(_cast_e5m2(dt, M, K))
    case("asq_cast_e5m2", f"{NAME[dt]}-unaligned-xq")(_cast_e5m2(dt, 3, 48, xq_skew=1))
    case("asq_cast_e5m2", f"{NAME[dt]}-unaligned-x")(_cast_e5m2(dt, 3, 48, x_skew=esize(dt)))


def _quantize_mxfp8(dt, M, K):
    def make():
        from autosmoothquant_amd import ops
        x = rnd(dt, (M, K), "mx")

        def call(r):
            return L.lib().asq_quantize_mxfp8(r.inp("x", x), CODE[dt], r.out("xq", (M, K), U8), r.out("scales", (M, K // 32), U8, 16, 1), M, K, r.stream)
        return call, lambda: dict(zip(("xq", "scales"), ops.quantize_mxfp8(x)))
    return make


for dt in FLOATS:
    for i, K in enumerate((32, 64, 32 * 255, 32 * 256, 32 * 257)):      # (one 32-element block per thread, 256 threads per block)
        case("asq_quantize_mxfp8", f"{NAME[dt]}-K{K}")(_quantize_mxfp8(dt, rows_for(i), K))
    for M in ROWS:
        case("asq_quantize_mxfp8", f"{NAME[dt]}-M{M}")(_quantize_mxfp8(dt, M, 96))


# ---- rope: dense, in place, and on the q / k slice of a fused q || k || v row -------------------------------------------------------------------
def _rope(dt, B, S, Hq, Hk, D, which):
    """which: "dense" | "inplace" | "q" | "k" (x = that slice of a [B, S, (Hq + 2 Hk) D] buffer)"""
    def make():
        from autosmoothquant_amd import ops
        H = Hk if which == "k" else Hq
        cos, sin = rnd(dt, (S, D // 2), "cos", scale=0.5), rnd(dt, (S, D // 2), "sin", scale=0.5)
        ld = (Hq + 2 * Hk) * D
        fused = rnd(dt, (B, S, ld), "qkv")
        lo = Hq * D if which == "k" else 0
        xs = fused[:, :, lo:lo + H * D].unflatten(-1, (H, D))                  # the strided slice
        xd = xs.contiguous()

        def call(r):
            pc, ps = r.inp("cos", cos), r.inp("sin", sin)
            if which in ("q", "k"):     # the whole fused buffer is the input region: v, the other slice and the slice itself must not change
                px = r.inp("qkv", fused) + lo * esize(dt)
                return L.lib().asq_rope(px, ld, r.out("out", (B, S, H, D), dt), CODE[dt], pc, ps, B, S, H, D, r.stream)
            if which == "inplace":
                po = r.out("out", (B, S, H, D), dt, init=xd)
                return L.lib().asq_rope(po, 0, po, CODE[dt], pc, ps, B, S, H, D, r.stream)
            return L.lib().asq_rope(r.inp("x", xd), 0, r.out("out", (B, S, H, D), dt), CODE[dt], pc, ps, B, S, H, D, r.stream)

        def ref():
            return {"out": ops.rope(xs if which in ("q", "k") else xd, cos, sin)}
        return call, ref
    return make


for dt in FLOATS:
    for which in ("dense", "inplace", "q", "k"):
        for (B, S, Hq, Hk, D) in ((1, 1, 1, 1, 16), (2, 3, 4, 2, 64), (1, 5, 3, 1, 128), (3, 67, 5, 2, 48)):
            case("asq_rope", f"{NAME[dt]}-{which}-B{B}S{S}H{Hq}+2x{Hk}D{D}")(_rope(dt, B, S, Hq, Hk, D, which))


def _weight_offset_image(N, K):
    def make():
        from autosmoothquant_amd import ops
        w = ri8((N, K), "woi")

        def call(r):
            return L.lib().asq_weight_offset_image(r.inp("w", w), N, K, r.out("w_off", (N, K), I8), r.out("col_off", (N, 2), I32), r.stream)
        return call, lambda: dict(zip(("w_off", "col_off"), ops.weight_offset_image(w)))
    return make


for (N, K) in ((4, 16), (8, 16 * 255), (12, 16 * 256), (4, 16 * 257), (4, 65536), (4100, 48)):
    case("asq_weight_offset_image", f"N{N}-K{K}")(_weight_offset_image(N, K))


# =====================================================================================================================================
# GEMM family
# =====================================================================================================================================
# per kernel name of asq_gemm_kernel_name: M and N one below, at and one above a multiple of its tile; K at one tile and at 2 or 3 (the
# generic kernel, 64 x 64 x 64: also one below / above)
GEMM_SHAPES = {
    "skinny": [(15, 63, 128), (16, 64, 256), (17, 65, 384), (1, 1, 128), (4, 33, 256)],            # 16-channel tiles, 4 / 8 / 16-row images
    "generic": [(63, 63, 63), (64, 64, 64), (65, 65, 65), (1, 1, 1), (5, 130, 129)],
    "p8q": [(383, 1535, 128), (384, 1536, 256), (385, 1537, 128)],                                 # 128 x 128
    "p8h": [(383, 511, 128), (384, 512, 256), (385, 513, 384)],                                    # 128 x 256
    "p16": [(2303, 4095, 128), (2304, 4096, 256), (2305, 4097, 128)],                              # 256 x 256, >= 144 tiles
}
FORCED_SHAPES = [(255, 511, 128), (256, 512, 256), (257, 513, 384), (300, 520, 1536)]              # p8 / p4 / p4x16 (256 x 256) and the K splits


def _expect_kernel(kern, M, N, K):
    name = L.lib().asq_gemm_kernel_name(M, N, K).decode()
    assert name == kern, f"the dispatcher sends {M} x {N} x {K} to '{name}', the case was written for '{kern}'"


def _gemm_ops(M, N, K, tag):
    x, w = ri8((M, K), "gx", tag), ri8((N, K), "gw", tag)
    return x, w, rpos((M,), "gsr", tag), rpos((N,), "gsc", tag, scale=1e-3), rnd(F32, (N,), "gb", tag, scale=1.0)


def _gemm_i32(kern, M, N, K, skew):
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w = ri8((M, K), "gx", kern), ri8((N, K), "gw", kern)

        def call(r):
            ws, n = r.ws(L.lib().asq_gemm_workspace_bytes(M, N, K))
            return L.lib().asq_gemm_i8_i32(r.inp("x", x), r.inp("w", w), r.out("out", (M, N), I32, 16, skew), M, N, K, ws, n, r.stream)
        return call, lambda: {"out": ops.gemm_i8_i32(x, w, torch.empty((M, N), dtype=I32, device=_dev()))}
    return make


def _gemm_i8(kern, M, N, K, skew, beta):
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w, c = ri8((M, K), "gx", kern), ri8((N, K), "gw", kern), ri8((M, N), "gc", kern)

        def call(r):
            ws, n = r.ws(L.lib().asq_gemm_workspace_bytes(M, N, K))
            po = r.out("out", (M, N), I8, 16, skew, init=c if beta else None)       # beta != 0: C == D in place
            return L.lib().asq_gemm_i8_i8(r.inp("x", x), r.inp("w", w), po, M, N, K, 3e-3, beta, ws, n, r.stream)
        return call, lambda: {"out": ops.gemm_i8_i8(x, w, c.clone(), 3e-3, beta)}
    return make


def _linear_w8a8(kern, M, N, K, dt, skew, variant):
    """variant 0: scalar scale; 1: s_row + bias; 2: s_col + bias, acc-first order"""
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w, sr, sc, b = _gemm_ops(M, N, K, kern)
        sr, sc, b = (None, None, None) if variant == 0 else (sr, None, b) if variant == 1 else (None, sc, b)
        order = "acc_first" if variant == 2 else "scale_first"

        def call(r):
            ws, n = r.ws(L.lib().asq_gemm_workspace_bytes(M, N, K))
            return L.lib().asq_linear_w8a8(r.inp("xq", x), r.inp("w", w), r.out("out", (M, N), dt, 16, skew), CODE[dt], M, N, K, 2e-3,
                                           r.inp("s_row", sr, 16, 4), r.inp("s_col", sc, 16, 4), r.inp("bias", b, 16, 4),
                                           L.ASQ_EPI_ACC_FIRST if variant == 2 else L.ASQ_EPI_SCALE_FIRST, ws, n, r.stream)
        return call, lambda: {"out": ops.linear_w8a8(x, w, dt, 2e-3, sr, sc, b, order)}
    return make


def _linear_q8(kern, M, N, K, mid, skew, act, qmode):
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w, sr, sc, b = _gemm_ops(M, N, K, kern)

        def call(r):
            ws, n = r.ws(L.lib().asq_gemm_workspace_bytes(M, N, K))
            return L.lib().asq_linear_w8a8_q8(r.inp("xq", x), r.inp("w", w), r.out("out", (M, N), I8, 16, skew), CODE[mid], M, N, K, 2e-3,
                                              r.inp("s_row", sr, 16, 4), None, r.inp("bias", b, 16, 4), L.ASQ_EPI_SCALE_FIRST, int(act),
                                              _MODES[qmode], 0.6, ws, n, r.stream)
        return call, lambda: {"out": ops.linear_w8a8_q8(x, w, mid, 2e-3, sr, None, b, "relu" if act else None, qmode, 0.6)}
    return make


_BIAS_DT = {0: (I32, I32), 1: (I32, I32), 2: (F32, F32), 3: (I8, I8), 4: (I8, I8)}


def _linear_i8_bias(kern, M, N, K, kind, skew):
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w = ri8((M, K), "gx", kern), ri8((N, K), "gw", kern)
        bdt, odt = _BIAS_DT[kind]
        bias = rnd(F32, (N,), "lb", scale=1.0) if bdt == F32 else torch.randint(-100, 100, (N,), generator=_gen("lb", N, kind), dtype=bdt).to(_dev())

        def call(r):
            ws, n = r.ws(L.lib().asq_gemm_workspace_bytes(M, N, K))
            return L.lib().asq_linear_i8_bias(r.inp("x", x), r.inp("w", w), r.inp("bias", bias, 16, esize(bdt)), r.out("out", (M, N), odt, 16, skew), kind,
                                              M, N, K, 4e-3, 0.75, ws, n, r.stream)
        return call, lambda: {"out": ops.linear_i8_bias(x, w, bias, kind, 4e-3, 0.75)}
    return make


def _forward(kern, M, N, K, dt, mode, skew, fused=False, image=False):
    def make():
        from autosmoothquant_amd import ops
        kern and _expect_kernel(kern, M, N, K)
        x, w = rnd(dt, (M, K), "fx", kern, scale=30.0), ri8((N, K), "gw", kern)
        sc, b = rpos((N,), "gsc", kern, scale=1e-3), rnd(F32, (N,), "gb", kern, scale=1.0)
        img = ops.weight_offset_image(w) if image else None

        def call(r):
            lib = L.lib()
            px, pw, po = r.inp("x", x), r.inp("w", w), r.out("out", (M, N), dt, 16, skew)
            psc, pb = r.inp("s_col", sc, 16, 4), r.inp("bias", b, 16, 4)
            if fused:
                return lib.asq_linear_w8a8_forward_fused(px, CODE[dt], pw, po, M, N, K, _MODES[mode], 0.8, 1.0, psc, pb, r.stream)
            ws, n = r.ws(lib.asq_linear_w8a8_workspace_bytes(M, N, K))
            if image:
                return lib.asq_linear_w8a8_forward_off(px, CODE[dt], pw, r.inp("w_off", img[0]), r.inp("col_off", img[1]), po, M, N, K, _MODES[mode], 0.8, 1.0,
                                                       psc, pb, ws, n, r.stream)
            return lib.asq_linear_w8a8_forward(px, CODE[dt], pw, po, M, N, K, _MODES[mode], 0.8, 1.0, psc, pb, ws, n, r.stream)

        def ref():
            if fused:
                return {"out": ops.linear_w8a8_forward_fused(x, w, mode, 0.8, 1.0, sc, b)}
            return {"out": ops.linear_w8a8_forward(x, w, mode, 0.8, 1.0, sc, b, image=img)}
        return call, ref
    return make


def _linear_off(M, N, K, dt, skew, variant):
    def make():
        from autosmoothquant_amd import ops
        _expect_kernel("p16", M, N, K)
        xf, w = rnd(F16, (M, K), "ox", scale=30.0), ri8((N, K), "gw", "off")
        xq, s_row, row_off = ops.quantize_act_off(xf, "per-token")
        w_off, col_off = ops.weight_offset_image(w)
        sc, b = rpos((N,), "gsc", "off", scale=1e-3), rnd(F32, (N,), "gb", "off", scale=1.0)
        sr, sc_, b_ = (s_row, None, b) if variant == 0 else (None, sc, None)

        def call(r):
            return L.lib().asq_linear_w8a8_off(r.inp("xq_off", xq), r.inp("w_off", w_off), r.out("out", (M, N), dt, 16, skew), CODE[dt], M, N, K, 2e-3,
                                               r.inp("s_row", sr, 16, 4), r.inp("s_col", sc_, 16, 4), r.inp("bias", b_, 16, 4), L.ASQ_EPI_SCALE_FIRST,
                                               r.inp("row_off", row_off, 16, 8), r.inp("col_off", col_off), r.stream)
        return call, lambda: {"out": ops.linear_w8a8_off(xq, w_off, row_off, col_off, dt, 2e-3, sr, sc_, b_)}
    return make


def _gate_up(M, F, K, dt, q8, images, fast):
    def make():
        from autosmoothquant_amd import ops
        assert L.lib().asq_gate_up_supported(M, F, K, CODE[dt]) == 1, (M, F, K)
        xf = rnd(F16, (M, K), "gux", scale=30.0)
        wgu = ops.interleave_gate_up(ri8((F, K), "gug"), ri8((F, K), "guu"))
        if images:
            xq, _, row_off = ops.quantize_act_off(xf, "per-tensor-round")
            wgu, col_off = ops.weight_offset_image(wgu)
        else:
            xq, row_off, col_off = ops.quantize_act(xf, "per-tensor-round")[0], None, None
        sr = rpos((M,), "gusr")

        def call(r):
            px, pw = r.inp("xq", xq), r.inp("w_gu", wgu)
            psr, pro, pco = r.inp("s_row", sr, 16, 4), r.inp("row_off", row_off, 16, 8), r.inp("col_off", col_off, 16, 8)
            if q8:
                return L.lib().asq_linear_w8a8_gate_up_q8(px, pw, r.out("out", (M, F), I8), CODE[dt], M, F, K, 1e-3, 2e-3, psr, 2 if fast else 0, 0.05, pro, pco, r.stream)
            return L.lib().asq_linear_w8a8_gate_up(px, pw, r.out("out", (M, F), dt), CODE[dt], M, F, K, 1e-3, 2e-3, psr, 2 if fast else 0, pro, pco, r.stream)

        def ref():
            if q8:
                return {"out": ops.linear_w8a8_gate_up_q8(xq, wgu, dt, 1e-3, 2e-3, 0.05, sr, fast, row_off, col_off)}
            return {"out": ops.linear_w8a8_gate_up(xq, wgu, dt, 1e-3, 2e-3, sr, fast, row_off, col_off)}
        return call, ref
    return make


def _linear_fp8(M, N, K, dt, skew, e5m2, variant):
    """variant 0: host scale, no bias; 1: per-token device scale + bias; 2: per-tensor device scale + bias"""
    def make():
        from autosmoothquant_amd import ops
        f8 = torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn
        xq, w = rf8((M, K), "f8x").to(F32).to(f8), rf8((N, K), "f8w").to(F32).to(f8)
        a = None if variant == 0 else rpos((M, 1), "f8a") if variant == 1 else rpos((), "f8a")
        b = None if variant == 0 else rnd(F32, (N,), "f8b", scale=1.0)

        def call(r):
            return L.lib().asq_linear_fp8(r.inp("xq", xq), r.inp("w", w), 1 if e5m2 else 0, r.out("out", (M, N), dt, 16, skew), CODE[dt], M, N, K,
                                          r.inp("a_scale", a, 16, 4), 1 if variant == 1 else 0, 0.013, 0.021, r.inp("bias", b, 16, 4 if variant == 1 else 0), r.stream)
        return call, lambda: {"out": ops.linear_fp8(xq, 0.013 if a is None else a, w, 0.021, b, dt)}
    return make


def _linear_mxfp8(M, N, K, dt, skew, bias):
    def make():
        from autosmoothquant_amd import ops
        xq, xs = ops.quantize_mxfp8(rnd(F16, (M, K), "mxx"))
        wq, wsc = ops.quantize_mxfp8(rnd(F16, (N, K), "mxw", scale=0.3))
        b = rnd(F32, (N,), "mxb", scale=1.0) if bias else None

        def call(r):
            return L.lib().asq_linear_mxfp8(r.inp("xq", xq), r.inp("x_scales", xs), r.inp("wq", wq), r.inp("w_scales", wsc),
                                            r.out("out", (M, N), dt, 16, skew), CODE[dt], M, N, K, r.inp("bias", b, 16, 4), r.stream)
        return call, lambda: {"out": ops.linear_mxfp8(xq, xs, wq, wsc, dt, b)}
    return make


def gemm_family(kern, shapes, group=None, big=False):
    """the int8 GEMM entries on `shapes` of one kernel; big: the 256 x 256 shapes (fewer variants: their outputs are tens of MB)"""
    for i, (M, N, K) in enumerate(shapes):
        tag = f"{kern}-{M}x{N}x{K}"
        sk = lambda e: e if i % 2 == 0 else 0          # noqa: E731  (the smallest alignment the entry admits on every other shape, 16 bytes on the rest)
        case("asq_gemm_i8_i32", tag, group)(_gemm_i32(kern, M, N, K, sk(4)))
        case("asq_gemm_i8_i8", tag, group)(_gemm_i8(kern, M, N, K, sk(1), 0.0))
        case("asq_linear_w8a8", f"{tag}-f16", group)(_linear_w8a8(kern, M, N, K, F16, sk(2), 1))
        case("asq_linear_w8a8", f"{tag}-f32", group)(_linear_w8a8(kern, M, N, K, F32, sk(4), 2))
        case("asq_linear_w8a8_q8", f"{tag}-f16-relu", group)(_linear_q8(kern, M, N, K, F16, sk(1), True, "per-tensor-div"))
        case("asq_linear_i8_bias", f"{tag}-kind{i % 5}", group)(_linear_i8_bias(kern, M, N, K, i % 5, sk(esize(_BIAS_DT[i % 5][1]))))
        case("asq_linear_w8a8_forward", f"{tag}-f16-pt", group)(_forward(kern, M, N, K, F16, "per-token", sk(2)))
        if not big:
            case("asq_gemm_i8_i8", f"{tag}-beta", group)(_gemm_i8(kern, M, N, K, sk(1), 0.5))
            case("asq_linear_w8a8", f"{tag}-bf16", group)(_linear_w8a8(kern, M, N, K, BF16, sk(2), 0))
            case("asq_linear_w8a8_q8", f"{tag}-bf16", group)(_linear_q8(kern, M, N, K, BF16, sk(1), False, "per-tensor-round"))
            for kind in range(5):
                if kind != i % 5:
                    case("asq_linear_i8_bias", f"{tag}-kind{kind}", group)(_linear_i8_bias(kern, M, N, K, kind, sk(esize(_BIAS_DT[kind][1]))))
            case("asq_linear_w8a8_forward", f"{tag}-bf16-round", group)(_forward(kern, M, N, K, BF16, "per-tensor-round", sk(2)))
            case("asq_linear_w8a8_forward", f"{tag}-f32-div", group)(_forward(kern, M, N, K, F32, "per-tensor-div", sk(4)))


for kern, shapes in GEMM_SHAPES.items():
    gemm_family(kern, shapes, big=kern == "p16")

# the K split of the 128 x 128 kernel, reduced in the launch: the only dispatcher-chosen path with GEMM scratch at a small size (12 MB)
for dt, skew in ((F16, 2), (F32, 0)):
    case("asq_linear_w8a8", f"p8q-ksplit-256x4096x4096-{NAME[dt]}")(_linear_w8a8("p8q", 256, 4096, 4096, dt, skew, 1))
case("asq_gemm_i8_i32", "p8q-ksplit-256x4096x4096")(_gemm_i32("p8q", 256, 4096, 4096, 4))
case("asq_linear_w8a8_forward", "p8q-ksplit-256x4096x4096-f16")(_forward("p8q", 256, 4096, 4096, F16, "per-token", 2))

# main launch + a column remainder of 128 x 128 tiles ("p16+tail": a few tiles over a round, K >= 4096), ragged M and N
TAIL_SHAPE = (1530, 11004, 4096)
case("asq_gemm_i8_i32", "p16+tail")(_gemm_i32("p16+tail", *TAIL_SHAPE, 4))
case("asq_linear_w8a8", "p16+tail-f16")(_linear_w8a8("p16+tail", *TAIL_SHAPE, F16, 2, 1))
case("asq_linear_w8a8_q8", "p16+tail-bf16")(_linear_q8("p16+tail", *TAIL_SHAPE, BF16, 1, False, "per-tensor-round"))

# the one-launch forward: 4 / 8 / 16-row activation images, 16-channel tiles
for i, (M, N, K) in enumerate(((1, 16, 128), (4, 15, 128), (5, 17, 256), (8, 33, 384), (9, 64, 128), (16, 65, 256), (3, 4096, 1024))):
    for dt, mode in ((F16, "per-token"), (BF16, "per-tensor-round"), (F32, "per-tensor-div")):
        case("asq_linear_w8a8_forward_fused", f"{M}x{N}x{K}-{NAME[dt]}-{mode}")(_forward(None, M, N, K, dt, mode, esize(dt) if i % 2 == 0 else 0, fused=True))
# ... and where asq_linear_w8a8_forward takes it by itself (asq_forward_fused_supported)
case("asq_linear_w8a8_forward", "fused-by-itself-4x768x1024-f16")(_forward("skinny", 4, 768, 1024, F16, "per-token", 2))

# offset operand images: always the 256 x 256 kernel
for i, (M, N, K) in enumerate(((2303, 4092, 128), (2304, 4096, 256), (2305, 4100, 128))):
    case("asq_linear_w8a8_off", f"{M}x{N}x{K}-f16")(_linear_off(M, N, K, F16, 2 if i % 2 == 0 else 0, 0))
    case("asq_linear_w8a8_off", f"{M}x{N}x{K}-f32")(_linear_off(M, N, K, F32, 4 if i % 2 == 0 else 0, 1))
    case("asq_linear_w8a8_forward_off", f"{M}x{N}x{K}-f16")(_forward("p16", M, N, K, F16, "per-token", 2 if i % 2 == 0 else 0, image=True))
case("asq_linear_w8a8_forward_off", "no-image-path-385x516x256-bf16")(_forward("p8h", 385, 516, 256, BF16, "per-tensor-round", 2, image=True))

# gate || up on the persistent 256 x 256 kernel: more than 256 tiles over [M, 2 F]
for i, (M, F, K) in enumerate(((4352, 2048, 256), (4352, 2176, 256), (4608, 2048, 512))):
    case("asq_linear_w8a8_gate_up", f"{M}x{F}x{K}-f16")(_gate_up(M, F, K, F16, False, False, True))
    case("asq_linear_w8a8_gate_up", f"{M}x{F}x{K}-bf16-images")(_gate_up(M, F, K, BF16, False, True, False))
    case("asq_linear_w8a8_gate_up_q8", f"{M}x{F}x{K}-f16")(_gate_up(M, F, K, F16, True, False, False))
    case("asq_linear_w8a8_gate_up_q8", f"{M}x{F}x{K}-bf16-images")(_gate_up(M, F, K, BF16, True, True, True))

# fp8 / MX: the same tile edges (launch_gemm picks among the same kernels; the MX kernels: 128 x 128 tiled for K % 512 == 0, 64 x 64 plain otherwise)
for kern in ("skinny", "p8q", "p8h", "p16"):
    for i, (M, N, K) in enumerate(GEMM_SHAPES[kern][:3]):
        dts = ((F16, 2),) if kern == "p16" else ((F16, 2), (F32, 4), (BF16, 0))
        for dt, skew in dts:
            case("asq_linear_fp8", f"{kern}-{M}x{N}x{K}-{NAME[dt]}")(_linear_fp8(M, N, K, dt, skew if i % 2 == 0 else 0, False, (i + skew) % 3))
    case("asq_linear_fp8", f"{kern}-e5m2")(_linear_fp8(*GEMM_SHAPES[kern][2], F16, 2, True, 1))
for i, (M, N, K) in enumerate(((127, 127, 512), (128, 128, 1024), (129, 129, 512), (63, 63, 64), (64, 64, 128), (65, 65, 192), (1, 1, 64), (5, 516, 512))):
    for dt, skew in ((F16, 2), (F32, 4), (BF16, 0)):
        case("asq_linear_mxfp8", f"{M}x{N}x{K}-{NAME[dt]}")(_linear_mxfp8(M, N, K, dt, skew if i % 2 == 0 else 0, i % 2 == 1))


# =====================================================================================================================================
# grouped and batched launches
# =====================================================================================================================================
GROUPS = ([300, 0, 17, 256, 1, 511], [0, 0, 5])


def _offsets(groups):
    o = [0]
    for g in groups:
        o.append(o[-1] + g)
    return torch.tensor(o, dtype=I32).to(_dev()), o[-1]


def _grouped(entry, groups, N, K, dt, pt, bias):
    def make():
        from autosmoothquant_amd import ops
        G = len(groups)
        goff, M = _offsets(groups)
        w = ri8((G, N, K), "grw")
        sg, b = rpos((G,), "grs"), (rnd(F32, (G, N), "grb", scale=1.0) if bias else None)
        xf = rnd(F16, (M, K), "grx", scale=30.0)
        if entry.endswith("_off"):
            xq, sr, row_off = ops.quantize_act_off(xf, "per-token" if pt else "per-tensor-round")
            w2, col_off = ops.weight_offset_image(w.view(G * N, K))
            w = w2.view(G, N, K)
        else:
            xq, sr = ops.quantize_act(xf, "per-token" if pt else "per-tensor-round")

        def call(r):
            lib = L.lib()
            px, pw, po = r.inp("xq", xq), r.inp("w", w), r.out("out", (M, N), dt, 16, 0)
            pg, psg, psr, pb = r.inp("group_offsets", goff, 16, 4), r.inp("s_group", sg, 16, 4), r.inp("s_row", sr, 16, 4), r.inp("bias", b, 16, 4)
            if entry == "asq_linear_w8a8_grouped":
                return lib.asq_linear_w8a8_grouped(px, pw, po, CODE[dt], pg, G, M, N, K, psg, psr, pb, r.stream)
            ws, n = r.ws(lib.asq_grouped_workspace_bytes(M, N, K, G))
            if entry == "asq_linear_w8a8_grouped_ws":
                return lib.asq_linear_w8a8_grouped_ws(px, pw, po, CODE[dt], pg, G, M, N, K, psg, psr, pb, ws, n, r.stream)
            return lib.asq_linear_w8a8_grouped_off(px, pw, po, CODE[dt], pg, G, M, N, K, psg, psr, pb, r.inp("row_off", row_off, 16, 8), r.inp("col_off", col_off, 16, 8),
                                                   ws, n, r.stream)

        def ref():
            if entry.endswith("_off"):
                return {"out": ops.linear_w8a8_grouped_off(xq, w, row_off, col_off, goff, sg, dt, sr, b)}
            return {"out": ops.linear_w8a8_grouped(xq, w, goff, sg, dt, sr, b)}
        return call, ref
    return make


def _grouped_gate_up(groups, F, K, dt, images, fast):
    def make():
        from autosmoothquant_amd import ops
        G = len(groups)
        goff, M = _offsets(groups)
        wgu = ops.interleave_gate_up_stack(ri8((G, F, K), "ggg"), ri8((G, F, K), "ggu"))
        s1, s3 = rpos((G,), "gg1", scale=2e-3), rpos((G,), "gg3", scale=2e-3)
        xf = rnd(F16, (M, K), "ggx", scale=30.0)
        if images:
            xq, _, row_off = ops.quantize_act_off(xf, "per-tensor-round")
            w2, col_off = ops.weight_offset_image(wgu.view(G * 2 * F, K))
            wgu = w2.view(G, 2 * F, K)
        else:
            xq, row_off, col_off = ops.quantize_act(xf, "per-tensor-round")[0], None, None

        def call(r):
            lib = L.lib()
            px, pw, po = r.inp("xq", xq), r.inp("w_gu", wgu), r.out("out", (M, F), dt)
            pg, p1, p3 = r.inp("group_offsets", goff, 16, 4), r.inp("s_gate", s1, 16, 4), r.inp("s_up", s3, 16, 4)
            pro, pco = r.inp("row_off", row_off, 16, 8), r.inp("col_off", col_off, 16, 8)
            ws, n = r.ws(lib.asq_grouped_workspace_bytes(M, 2 * F, K, G))
            return lib.asq_linear_w8a8_grouped_gate_up(px, pw, po, CODE[dt], pg, G, M, F, K, p1, p3, 2 if fast else 0, pro, pco, ws, n, r.stream)
        return call, lambda: {"out": ops.linear_w8a8_grouped_gate_up(xq, wgu, goff, s1, s3, dt, fast, row_off, col_off)}
    return make


def _fp8_grouped(groups, N, K, dt, bias, gate_up, fast=False):
    def make():
        from autosmoothquant_amd import ops
        G = len(groups)
        goff, M = _offsets(groups)
        xq, a = ops.quantize_act_fp8(rnd(F16, (M, K), "fgx"), "per-token")
        a = a.reshape(M).contiguous()
        if gate_up:
            w = ops.interleave_gate_up_stack(rf8((G, N, K), "fg1"), rf8((G, N, K), "fg3"))
            s1, s3 = rpos((G,), "fgs1"), rpos((G,), "fgs3")
        else:
            w, s1, b = rf8((G, N, K), "fgw"), rpos((G,), "fgs"), (rnd(F32, (G, N), "fgb", scale=1.0) if bias else None)

        def call(r):
            lib = L.lib()
            px, pw, po = r.inp("xq", xq), r.inp("w", w), r.out("out", (M, N), dt, 16, 0)
            pg, pa, p1 = r.inp("group_offsets", goff, 16, 4), r.inp("a_scale", a, 16, 4), r.inp("s1", s1, 16, 4)
            if gate_up:
                return lib.asq_linear_fp8_grouped_gate_up(px, pw, po, CODE[dt], pg, G, M, N, K, pa, p1, r.inp("s3", s3, 16, 4), 2 if fast else 0, r.stream)
            return lib.asq_linear_fp8_grouped(px, pw, po, CODE[dt], pg, G, M, N, K, pa, p1, r.inp("bias", b, 16, 4), r.stream)

        def ref():
            if gate_up:
                return {"out": ops.linear_fp8_grouped_gate_up(xq, a, w, goff, s1, s3, dt, fast)}
            return {"out": ops.linear_fp8_grouped(xq, a, w, s1, goff, dt, b)}
        return call, ref
    return make


for gi, groups in enumerate(GROUPS):
    gname = "x".join(map(str, groups))
    # K = 256: no workspace for this shape; K = 4096: the tail round's K split with exactly asq_grouped_workspace_bytes (header + 64 MiB)
    for (N, K) in ((260, 256), (384, 4096)):
        for dt in (F16, F32) if K == 256 else (BF16,):
            case("asq_linear_w8a8_grouped", f"{gname}-N{N}K{K}-{NAME[dt]}")(_grouped("asq_linear_w8a8_grouped", groups, N, K, dt, True, True))
            case("asq_linear_w8a8_grouped_ws", f"{gname}-N{N}K{K}-{NAME[dt]}")(_grouped("asq_linear_w8a8_grouped_ws", groups, N, K, dt, False, dt != F32))
            if dt != F32:
                case("asq_linear_w8a8_grouped_off", f"{gname}-N{N}K{K}-{NAME[dt]}")(_grouped("asq_linear_w8a8_grouped_off", groups, N, K, dt, True, K == 256))
    for (F, K) in ((128, 256), (384, 4096)):
        case("asq_linear_w8a8_grouped_gate_up", f"{gname}-F{F}K{K}-f16")(_grouped_gate_up(groups, F, K, F16, False, True))
        case("asq_linear_w8a8_grouped_gate_up", f"{gname}-F{F}K{K}-bf16-images")(_grouped_gate_up(groups, F, K, BF16, True, False))
    for (N, K) in ((260, 256), (513, 128)):
        for dt in FLOATS:
            case("asq_linear_fp8_grouped", f"{gname}-N{N}K{K}-{NAME[dt]}")(_fp8_grouped(groups, N, K, dt, dt != BF16, False))
    for (F, K) in ((128, 256), (384, 128)):
        case("asq_linear_fp8_grouped_gate_up", f"{gname}-F{F}K{K}-f16")(_fp8_grouped(groups, F, K, F16, False, True, True))
        case("asq_linear_fp8_grouped_gate_up", f"{gname}-F{F}K{K}-bf16")(_fp8_grouped(groups, F, K, BF16, False, True, False))


_BMM_DT = {L.ASQ_BMM_S32: I32, L.ASQ_BMM_F32: F32, L.ASQ_BMM_S8: I8}


def _bmm(kind, B, M, N, K, skew, in_skew=0):
    def make():
        from autosmoothquant_amd import ops
        a, b = ri8((B, M, K), "bma"), ri8((B, N, K), "bmb")
        want = "m16" if M <= 16 else "t128"
        assert L.lib().asq_bmm_kernel_name(B, M, N, K, kind).decode() == want

        def call(r):
            return L.lib().asq_bmm_i8(r.inp("a", a, 16, in_skew), r.inp("b", b, 16, in_skew), r.out("out", (B, M, N), _BMM_DT[kind], 16, skew), kind, B, M, N, K, 5e-3, r.stream)
        return call, lambda: {"out": ops.bmm_i8(a, b, kind, 5e-3)}
    return make


for kind, dt in _BMM_DT.items():
    for B in (1, 3, 17):
        for i, (M, N, K) in enumerate(((1, 63, 64), (15, 64, 48), (16, 65, 80), (5, 130, 17), (129, 127, 64), (129, 129, 33), (129, 128, 128))):
            case("asq_bmm_i8", f"{NAME[dt]}-B{B}-{M}x{N}x{K}")(_bmm(kind, B, M, N, K, esize(dt) if (i + B) % 2 == 0 else 0, 1 if i == 1 else 0))


case("asq_bmm_i8", "f32-K0")(_bmm(L.ASQ_BMM_F32, 3, 5, 7, 0, 4))         # K = 0 is not "nothing to do": the header has it write alpha * 0.0
case("asq_linear_i8_bias", "K0-kind2")(_linear_i8_bias(None, 5, 7, 0, 2, 4))
case("asq_gemm_i8_i32", "K0")(_gemm_i32(None, 5, 7, 0, 4))
case("asq_gemm_i8_i8", "K0")(_gemm_i8(None, 5, 7, 0, 1, 0.5))
case("asq_linear_w8a8", "K0-f16")(_linear_w8a8(None, 5, 7, 0, F16, 2, 1))


# =====================================================================================================================================
# asq_workspace_init: the header and nothing else
# =====================================================================================================================================
def _workspace_init(extra):
    def make():
        n = L.lib().asq_workspace_header_bytes() + extra

        def call(r):
            reg = r.arena.place(n, 256, 0, "workspace", "workspace")
            r.outs["workspace"] = (reg, U8, (n,))
            return L.lib().asq_workspace_init(reg.ptr, n, r.stream)

        def ref():   # the same call on an ordinary tensor that starts from the same bytes (the pattern at arena offset guard_bytes())
            t = GB.pattern(GB.guard_bytes(), n, _dev())
            L.check(L.lib().asq_workspace_init(t.data_ptr(), n, _stream()), "asq_workspace_init")
            return {"workspace": t}
        return call, ref
    return make


for extra in (0, 1, 1 << 20):
    case("asq_workspace_init", f"header+{extra}")(_workspace_init(extra))


# =====================================================================================================================================
# nothing to do: an empty problem leaves every output byte at its pattern
# =====================================================================================================================================
def _empty(entry, cid, fn):
    """fn(r, P) -> rc, with P(name) -> pointer of a pattern-filled 256-byte output region"""
    def make():
        def call(r):
            def P(name, nbytes=256, align=256):
                return r.out(name, (nbytes,), U8, align)
            return fn(r, P)

        def ref():
            return None
        return call, ref
    CASES.append(Case(entry, f"{entry}-empty-{cid}", make))


def run_empty(c):
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


def _i(r, name, n=256):
    """a small int8 input to point at"""
    return r.inp(name, torch.zeros((n,), dtype=I8, device=_dev()))


def _f(r, name, dt=F16, n=128):
    return r.inp(name, torch.ones((n,), dtype=dt, device=_dev()))


def _g(r, offs):
    return r.inp("group_offsets", torch.tensor(offs, dtype=I32).to(_dev()), 16, 4)


lib_ = L.lib   # (resolved when a case runs)
_empty("asq_gemm_i8_i32", "M0", lambda r, P: lib_().asq_gemm_i8_i32(_i(r, "x"), _i(r, "w"), P("out"), 0, 64, 128, None, 0, r.stream))
_empty("asq_gemm_i8_i32", "N0", lambda r, P: lib_().asq_gemm_i8_i32(_i(r, "x"), _i(r, "w"), P("out"), 2, 0, 128, None, 0, r.stream))
_empty("asq_gemm_i8_i8", "M0", lambda r, P: lib_().asq_gemm_i8_i8(_i(r, "x"), _i(r, "w"), P("out"), 0, 64, 128, 1.0, 0.0, None, 0, r.stream))
_empty("asq_quantize_act", "M0", lambda r, P: lib_().asq_quantize_act(_f(r, "x"), L.ASQ_F16, L.ASQ_ACT_PER_TOKEN, 1.0, P("xq"), P("s_row"), 0, 64, r.stream))
_empty("asq_quantize_act", "K0", lambda r, P: lib_().asq_quantize_act(_f(r, "x"), L.ASQ_F16, L.ASQ_ACT_ROUND, 1.0, P("xq"), None, 4, 0, r.stream))
_empty("asq_quantize_act_off", "M0", lambda r, P: lib_().asq_quantize_act_off(_f(r, "x"), L.ASQ_F16, L.ASQ_ACT_PER_TOKEN, 1.0, P("xq"), P("s_row"), P("row_off"), 0, 64, r.stream))
_empty("asq_weight_offset_image", "N0", lambda r, P: lib_().asq_weight_offset_image(_i(r, "w"), 0, 64, P("w_off"), P("col_off"), r.stream))
_empty("asq_norm_quantize", "M0", lambda r, P: lib_().asq_norm_quantize(_f(r, "x"), L.ASQ_F16, _f(r, "w"), None, 1e-5, 1, P("xq"), P("s_row"), 0, 64, r.stream))
_empty("asq_norm_quantize_off", "M0", lambda r, P: lib_().asq_norm_quantize_off(_f(r, "x"), L.ASQ_F16, _f(r, "w"), None, 1e-5, 1, P("xq"), P("s_row"), P("row_off"), 0, 64, r.stream))
_empty("asq_add_norm_quantize", "M0", lambda r, P: lib_().asq_add_norm_quantize(_f(r, "x"), _f(r, "res"), P("h"), L.ASQ_F16, _f(r, "w"), None, 1e-5, 1, P("xq"), P("s_row"), 0, 64, r.stream))
_empty("asq_add_norm_quantize_off", "M0", lambda r, P: lib_().asq_add_norm_quantize_off(_f(r, "x"), _f(r, "res"), P("h"), L.ASQ_F16, _f(r, "w"), None, 1e-5, 1, P("xq"), P("s_row"), P("row_off"), 0, 64, r.stream))
_empty("asq_dq_add_layernorm_q", "M0", lambda r, P: lib_().asq_dq_add_layernorm_q(_f(r, "x", F32), 1.0, _f(r, "res"), P("h"), L.ASQ_F16, _f(r, "g"), _f(r, "b"), 1e-5, P("q"), 0, 64, r.stream))
_empty("asq_silu_mul_quantize", "M0", lambda r, P: lib_().asq_silu_mul_quantize(_f(r, "g"), _f(r, "u"), L.ASQ_F16, 1, 1.0, P("xq"), P("s_row"), 0, 64, r.stream))
_empty("asq_silu_mul_quantize_off", "M0", lambda r, P: lib_().asq_silu_mul_quantize_off(_f(r, "g"), _f(r, "u"), L.ASQ_F16, 1, 1.0, P("xq"), P("s_row"), P("row_off"), 0, 64, r.stream))
_empty("asq_silu_mul_quantize_fp8", "M0", lambda r, P: lib_().asq_silu_mul_quantize_fp8(_f(r, "g"), _f(r, "u"), L.ASQ_F16, 0, P("xq"), P("scale"), 0, 64, r.stream))
_empty("asq_rmsnorm", "M0", lambda r, P: lib_().asq_rmsnorm(_f(r, "x"), L.ASQ_F16, _f(r, "w"), 1e-5, P("y"), 0, 64, r.stream))
_empty("asq_silu_mul", "n0", lambda r, P: lib_().asq_silu_mul(_f(r, "g"), _f(r, "u"), L.ASQ_F16, 0, P("out"), 0, r.stream))
_empty("asq_rope", "B0", lambda r, P: lib_().asq_rope(_f(r, "x"), 0, P("out"), L.ASQ_F16, _f(r, "cos"), _f(r, "sin"), 0, 4, 1, 16, r.stream))
_empty("asq_rope", "S0", lambda r, P: lib_().asq_rope(_f(r, "x"), 0, P("out"), L.ASQ_F16, _f(r, "cos"), _f(r, "sin"), 2, 0, 1, 16, r.stream))
_empty("asq_rope", "H0", lambda r, P: lib_().asq_rope(_f(r, "x"), 0, P("out"), L.ASQ_F16, _f(r, "cos"), _f(r, "sin"), 2, 4, 0, 16, r.stream))
_empty("asq_linear_w8a8", "M0", lambda r, P: lib_().asq_linear_w8a8(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 0, 64, 128, 1.0, None, None, None, 0, None, 0, r.stream))
_empty("asq_linear_w8a8", "N0", lambda r, P: lib_().asq_linear_w8a8(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 2, 0, 128, 1.0, None, None, None, 0, None, 0, r.stream))
_empty("asq_linear_w8a8_q8", "M0", lambda r, P: lib_().asq_linear_w8a8_q8(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 0, 64, 128, 1.0, None, None, None, 0, 0, 0, 1.0, None, 0, r.stream))
_empty("asq_linear_w8a8_off", "M0", lambda r, P: lib_().asq_linear_w8a8_off(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 0, 64, 128, 1.0, None, None, None, 0, _f(r, "ro", F32), _f(r, "co", F32), r.stream))
_empty("asq_linear_w8a8_forward", "M0", lambda r, P: lib_().asq_linear_w8a8_forward(_f(r, "x"), L.ASQ_F16, _i(r, "w"), P("out"), 0, 64, 128, 2, 1.0, 1.0, None, None, None, 0, r.stream))
_empty("asq_linear_w8a8_forward_off", "M0", lambda r, P: lib_().asq_linear_w8a8_forward_off(_f(r, "x"), L.ASQ_F16, _i(r, "w"), None, None, P("out"), 0, 64, 128, 2, 1.0, 1.0, None, None, None, 0, r.stream))
_empty("asq_linear_w8a8_forward_fused", "M0", lambda r, P: lib_().asq_linear_w8a8_forward_fused(_f(r, "x"), L.ASQ_F16, _i(r, "w"), P("out"), 0, 64, 128, 2, 1.0, 1.0, None, None, r.stream))
_empty("asq_linear_w8a8_gate_up", "M0", lambda r, P: lib_().asq_linear_w8a8_gate_up(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 0, 128, 256, 1.0, 1.0, None, 0, None, None, r.stream))
_empty("asq_linear_w8a8_gate_up_q8", "M0", lambda r, P: lib_().asq_linear_w8a8_gate_up_q8(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, 0, 128, 256, 1.0, 1.0, None, 0, 1.0, None, None, r.stream))
_empty("asq_linear_w8a8_grouped", "M0", lambda r, P: lib_().asq_linear_w8a8_grouped(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 64, 128, _f(r, "sg", F32), None, None, r.stream))
_empty("asq_linear_w8a8_grouped_ws", "M0", lambda r, P: lib_().asq_linear_w8a8_grouped_ws(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 64, 128, _f(r, "sg", F32), None, None, None, 0, r.stream))
_empty("asq_linear_w8a8_grouped_off", "M0", lambda r, P: lib_().asq_linear_w8a8_grouped_off(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 64, 128, _f(r, "sg", F32), None, None, None, None, None, 0, r.stream))
_empty("asq_linear_w8a8_grouped_gate_up", "M0", lambda r, P: lib_().asq_linear_w8a8_grouped_gate_up(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 128, 128, _f(r, "s1", F32), _f(r, "s3", F32), 0, None, None, None, 0, r.stream))
_empty("asq_quantize_act_fp8", "M0", lambda r, P: lib_().asq_quantize_act_fp8(_f(r, "x"), L.ASQ_F16, L.ASQ_FP8_PER_TOKEN, 1.0, P("xq"), P("scale"), 0, 64, r.stream))
_empty("asq_quantize_act_fp8", "K0-static", lambda r, P: lib_().asq_quantize_act_fp8(_f(r, "x"), L.ASQ_F16, L.ASQ_FP8_STATIC, 1.0, P("xq"), None, 4, 0, r.stream))
_empty("asq_linear_fp8", "M0", lambda r, P: lib_().asq_linear_fp8(_i(r, "x"), _i(r, "w"), 0, P("out"), L.ASQ_F16, 0, 64, 128, None, 0, 1.0, 1.0, None, r.stream))
_empty("asq_linear_fp8", "N0", lambda r, P: lib_().asq_linear_fp8(_i(r, "x"), _i(r, "w"), 0, P("out"), L.ASQ_F16, 2, 0, 128, None, 0, 1.0, 1.0, None, r.stream))
_empty("asq_linear_fp8_grouped", "M0", lambda r, P: lib_().asq_linear_fp8_grouped(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 64, 128, _f(r, "a", F32), _f(r, "s", F32), None, r.stream))
_empty("asq_linear_fp8_grouped_gate_up", "M0", lambda r, P: lib_().asq_linear_fp8_grouped_gate_up(_i(r, "x"), _i(r, "w"), P("out"), L.ASQ_F16, _g(r, [0, 0, 0]), 2, 0, 128, 128, _f(r, "a", F32), _f(r, "s1", F32), _f(r, "s3", F32), 0, r.stream))
_empty("asq_cast_e5m2", "n0", lambda r, P: lib_().asq_cast_e5m2(_f(r, "x"), L.ASQ_F16, P("xq"), 0, r.stream))
_empty("asq_quantize_mxfp8", "M0", lambda r, P: lib_().asq_quantize_mxfp8(_f(r, "x"), L.ASQ_F16, P("xq"), P("scales"), 0, 64, r.stream))
_empty("asq_quantize_mxfp8", "K0", lambda r, P: lib_().asq_quantize_mxfp8(_f(r, "x"), L.ASQ_F16, P("xq"), P("scales"), 4, 0, r.stream))
_empty("asq_linear_mxfp8", "M0", lambda r, P: lib_().asq_linear_mxfp8(_i(r, "x"), _i(r, "xs"), _i(r, "w"), _i(r, "ws"), P("out"), L.ASQ_F16, 0, 64, 64, None, r.stream))
_empty("asq_linear_mxfp8", "N0", lambda r, P: lib_().asq_linear_mxfp8(_i(r, "x"), _i(r, "xs"), _i(r, "w"), _i(r, "ws"), P("out"), L.ASQ_F16, 2, 0, 64, None, r.stream))
for _kind in (0, 1, 2):
    _empty("asq_bmm_i8", f"batch0-kind{_kind}", lambda r, P, k=_kind: lib_().asq_bmm_i8(_i(r, "a"), _i(r, "b"), P("out"), k, 0, 4, 4, 16, 1.0, r.stream))
    _empty("asq_bmm_i8", f"M0-kind{_kind}", lambda r, P, k=_kind: lib_().asq_bmm_i8(_i(r, "a"), _i(r, "b"), P("out"), k, 2, 0, 4, 16, 1.0, r.stream))
    _empty("asq_bmm_i8", f"N0-kind{_kind}", lambda r, P, k=_kind: lib_().asq_bmm_i8(_i(r, "a"), _i(r, "b"), P("out"), k, 2, 4, 0, 16, 1.0, r.stream))
for _kind in range(5):
    _empty("asq_linear_i8_bias", f"M0-kind{_kind}", lambda r, P, k=_kind: lib_().asq_linear_i8_bias(_i(r, "x"), _i(r, "w"), _i(r, "bias"), P("out"), k, 0, 64, 128, 1.0, 1.0, None, 0, r.stream))
    _empty("asq_linear_i8_bias", f"N0-kind{_kind}", lambda r, P, k=_kind: lib_().asq_linear_i8_bias(_i(r, "x"), _i(r, "w"), _i(r, "bias"), P("out"), k, 2, 0, 128, 1.0, 1.0, None, 0, r.stream))


# =====================================================================================================================================
# paths only an environment switch reaches: child processes, one per setting (the switches are read once per process)
# =====================================================================================================================================
# (p8, p4 and p4x16 are the kernel names no shape reaches by itself; the others have their dispatcher-chosen cases above)
for _kern in ("p8", "p4", "p4x16"):
    gemm_family(_kern, FORCED_SHAPES[:3], group=f"kernel-{_kern}")
for _kern in ("p8q", "p8h", "p8"):       # forced K splits: int32 slabs / register images in a workspace of exactly asq_gemm_workspace_bytes
    gemm_family(_kern, [FORCED_SHAPES[3], (257, 513, 1024)], group=f"ksplit-{_kern}")
gemm_family("p8q", GEMM_SHAPES["p8q"], group="mma32")
gemm_family("p8h", GEMM_SHAPES["p8h"], group="mma32")
for _gi, _groups in enumerate(GROUPS):
    FORCED["mma32"].append(Case("asq_linear_w8a8_grouped_ws", f"mma32-grouped-{_gi}", _grouped("asq_linear_w8a8_grouped_ws", _groups, 260, 4096, F16, True, True)))
gemm_family("p16", [TAIL_SHAPE], group="no-tail", big=True)
FORCED["fused-forward-off"] = [Case("asq_linear_w8a8_forward", f"fused-forward-off-{M}", _forward("skinny", M, 768, 1024, F16, "per-token", 2)) for M in (1, 4, 16)]

CHILDREN = [   # (id, group, environment, time limit in seconds)
    *[(f"kernel-{k}", f"kernel-{k}", {"ASQ_GEMM_KERNEL": k}, 240) for k in ("p8", "p4", "p4x16")],
    *[(f"ksplit{n}-{k}-fix{fix}", f"ksplit-{k}", {"ASQ_GEMM_KERNEL": k, "ASQ_KSPLIT": str(n), "ASQ_SPLITK_FIX": str(fix)}, 240)
      for (k, n, fix) in (("p8q", 3, 1), ("p8q", 4, 0), ("p8h", 3, 1), ("p8", 2, 1))],
    ("mma32", "mma32", {"ASQ_MMA": "32"}, 240),
    ("no-tail", "no-tail", {"ASQ_NO_TAIL": "1"}, 240),
    ("gate-up-off", "gate-up-off", {"ASQ_GATE_UP": "0"}, 240),
    ("fused-forward-off", "fused-forward-off", {"ASQ_FUSED_FORWARD": "0"}, 240),
]
_child_lost = []     # a child that ended on a signal or on its time limit: no further child is started


def child_main(group):
    """entry of a child process: run the group's cases in this process (its environment carries the switch)"""
    assert torch.cuda.is_available()
    if group == "gate-up-off":
        return child_gate_up_off()
    for c in FORCED[group]:
        run_case(c)
    print(f"guardband child ok: {group}, {len(FORCED[group])} cases")


def child_gate_up_off():
    """ASQ_GATE_UP=0 (include/asq_hip.h: "makes the query return 0"; "other shapes return ASQ_ERR_DIM (callers run the two linears + asq_silu_mul_quantize)"):
    the entries refuse a shape they would otherwise run, and write nothing."""
    M, F, K = 4352, 2048, 256
    lib = L.lib()
    assert lib.asq_gate_up_supported(M, F, K, L.ASQ_F16) == 0
    xq, w = ri8((M, K), "guoff-x"), ri8((2 * F, K), "guoff-w")
    for q8 in (False, True):
        run = Run(arena(), 0x7F)
        px, pw, po = run.inp("xq", xq), run.inp("w_gu", w), run.out("out", (M, F), I8 if q8 else F16)
        if q8:
            rc = lib.asq_linear_w8a8_gate_up_q8(px, pw, po, L.ASQ_F16, M, F, K, 1e-3, 2e-3, None, 0, 0.05, None, None, run.stream)
        else:
            rc = lib.asq_linear_w8a8_gate_up(px, pw, po, L.ASQ_F16, M, F, K, 1e-3, 2e-3, None, 0, None, None, run.stream)
        assert rc == ASQ_ERR_DIM, rc
        torch.cuda.synchronize()
        reg = run.outs["out"][0]
        assert torch.equal(reg.bytes(), GB.pattern(reg.off, reg.nbytes, _dev())), "a refused call wrote into its output"
        rep = run.arena.check()
        assert rep.ok, str(rep)
    print("guardband child ok: gate-up-off")


# =====================================================================================================================================
# the tests
# =====================================================================================================================================
@pytest.mark.parametrize("c", [c for c in CASES if "-empty-" not in c.id], ids=lambda c: c.id)
def test_entry_writes_only_its_outputs(c):
    run_case(c)


@pytest.mark.parametrize("c", [c for c in CASES if "-empty-" in c.id], ids=lambda c: c.id)
def test_nothing_to_do_leaves_every_output_byte(c):
    run_empty(c)


@pytest.mark.parametrize("cid,group,env,limit", CHILDREN, ids=[c[0] for c in CHILDREN])
def test_switched_paths_in_a_child_process(cid, group, env, limit):
    if _child_lost:
        pytest.fail(f"not started: the child '{_child_lost[0]}' ended on a signal or on its time limit")
    code = f"import sys; sys.path.insert(0, {ROOT!r}); sys.path.insert(0, {os.path.join(ROOT, 'tests')!r}); import test_hip_guardband as t; t.child_main({group!r})"
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        _child_lost.append(cid)
        pytest.fail(f"child '{cid}' exceeded its {limit} s: {str(e.stdout)[-1500:]}")
    if r.returncode < 0:
        _child_lost.append(cid)
    assert r.returncode == 0 and "guardband child ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_python_out_parameters_stay_inside_the_view():
    """each ops.* function with an out= parameter, given a view into the arena: the same five checks"""
    from autosmoothquant_amd import ops
    M, N, K = 300, 520, 256
    x, w, sr, sc, b = _gemm_ops(M, N, K, "py")
    xf = rnd(F16, (2304, K), "pyx", scale=30.0)
    wl = ri8((4096, K), "pyw")
    xq_off, s_off, row_off = ops.quantize_act_off(xf, "per-token")
    img = ops.weight_offset_image(wl)
    wg, wu = ri8((2048, K), "pyg"), ri8((2048, K), "pyu")
    wgu = ops.interleave_gate_up(wg, wu)
    xq_big = ri8((4352, K), "pyxq")
    res, h, nw = rnd(F16, (M, K), "pyres"), rnd(F16, (M, K), "pyh"), rnd(F16, (K,), "pynw", scale=1.0)
    rx, cos, sin = rnd(F16, (2, 5, 3, 64), "pyrope"), rnd(F16, (5, 32), "pycos", scale=0.5), rnd(F16, (5, 32), "pysin", scale=0.5)
    w1, w3 = ri8((3, 32, 48), "pyw1"), ri8((3, 32, 48), "pyw3")

    def view(r, name, shape, dt, skew=0, init=None):
        r.out(name, shape, dt, 16, skew, init=init)
        reg = r.outs[name][0]
        return reg.view(dt, shape)

    calls = {
        "linear_w8a8": (lambda r: ops.linear_w8a8(x, w, F16, 2e-3, sr, None, b, out=view(r, "out", (M, N), F16, 2)),
                        lambda: {"out": ops.linear_w8a8(x, w, F16, 2e-3, sr, None, b)}),
        "linear_w8a8_off": (lambda r: ops.linear_w8a8_off(xq_off, img[0], row_off, img[1], F16, 2e-3, s_off, None, None, out=view(r, "out", (2304, 4096), F16, 2)),
                            lambda: {"out": ops.linear_w8a8_off(xq_off, img[0], row_off, img[1], F16, 2e-3, s_off, None, None)}),
        "linear_w8a8_gate_up": (lambda r: ops.linear_w8a8_gate_up(xq_big, wgu, F16, 1e-3, 2e-3, out=view(r, "out", (4352, 2048), F16)),
                                lambda: {"out": ops.linear_w8a8_gate_up(xq_big, wgu, F16, 1e-3, 2e-3)}),
        "add_norm_quantize": (lambda r: ops.add_norm_quantize(h, res, nw, None, 1e-5, True, out=view(r, "h", (M, K), F16, 0, init=res)),
                              lambda: {"h": ops.add_norm_quantize(h, res, nw, None, 1e-5, True)[0]}),
        "rope": (lambda r: ops.rope(view(r, "out", (2, 5, 3, 64), F16, 0, init=rx), cos, sin, out=r.outs["out"][0].view(F16, (2, 5, 3, 64))),
                 lambda: {"out": ops.rope(rx, cos, sin)}),
        "weight_offset_image": (lambda r: ops.weight_offset_image(wl, out=(view(r, "w_off", (4096, K), I8), view(r, "col_off", (4096, 2), I32))),
                                lambda: dict(zip(("w_off", "col_off"), img))),
        "interleave_gate_up": (lambda r: ops.interleave_gate_up(wg, wu, out=view(r, "out", (4096, K), I8, 1)),
                               lambda: {"out": wgu}),
        "interleave_gate_up_stack": (lambda r: ops.interleave_gate_up_stack(w1, w3, out=view(r, "out", (3, 64, 48), I8, 1)),
                                     lambda: {"out": ops.interleave_gate_up_stack(w1, w3)}),
    }
    import inspect
    with_out = sorted(n for n, f in inspect.getmembers(ops, inspect.isfunction) if not n.startswith("_") and getattr(inspect.signature(f).parameters.get("out"), "default", 0) is None)
    assert with_out == sorted(calls), (with_out, sorted(calls))
    for name, (call, ref) in calls.items():
        run_case(Case(name, f"ops.{name}(out=)", lambda call=call, ref=ref: (lambda r: (call(r), 0)[1], ref)))


def test_the_gpu_path_of_the_helper_is_live():
    """a one-byte store into a guard, made with a torch index, is reported with its region, side and offset"""
    a = arena()
    a.reset(0x7F)
    x = a.place(1000, 16, 8, "input", "x", data=torch.zeros((1000,), dtype=U8, device=_dev()))
    y = a.place(4096, 16, 2, "output", "y", pitch=64)
    assert a.check().ok
    a.buf[y.off + y.nbytes] ^= 0x01
    a.buf[x.off - 1] ^= 0x80
    a.buf[x.off + 17] = 9
    rep = a.check()
    assert [(g["region"], g["side"], g["first"], g["last"]) for g in rep.guards] == [("x", "before", -1, -1), ("y", "after", 4096, 4096)], str(rep)
    assert [(i["region"], i["first"], i["last"]) for i in rep.inputs] == [("x", 17, 17)], str(rep)
