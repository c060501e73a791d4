"""The K ladders of the row kernels (csrc/asq_quant.hip, csrc/asq_fp8.hip) and the inputs that walk them: shared by the guard-band sweep
(tests/test_hip_guardband.py), the oracle comparison of every tier (tests/test_hip_row_ladders.py) and their CPU checks
(tests/test_row_ladders_cpu.py).  Nothing here touches a device.

Each launcher picks a template instantiation from nvec = K / VEC (VEC = 8 for fp16 / bf16, 4 for fp32):

    launcher                                              tier rule          tiers
    launch_rows_wave (plain and offset images)            ceil(nvec / 64)    WAVE_I8  (28: per-token rows only)
    quant_per_token_cached                                block per row      PT_BLOCK, then quant_per_token_generic
    quant_rows_off                                        block per row      OFF_BLOCK
    norm_quant_cached (ADD = 0 / 1 / 2), rmsnorm_rows     block per row      NORM
    silu_mul_quant_cached, silu_mul_quant_fp8_cached      block per row      SILU
    launch_fp8_rows_wave                                  ceil(nvec / 64)    WAVE_F8

tests/test_row_ladders_cpu.py reads the launch macros of the two sources and fails when a tuple below no longer matches them."""
import numpy as np

import detrng
from oracle import w8a8 as O

VEC = {"f32": 4, "f16": 8, "bf16": 8}
DTS = ("f16", "bf16", "f32")

WAVE_I8 = (1, 2, 4, 6, 8, 10, 12, 16, 22, 24, 28)      # launch_rows_wave: nv = ceil(K / VEC / 64)
WAVE_F8 = (1, 2, 4, 8, 12, 16, 22, 28)                 # launch_fp8_rows_wave
PT_BLOCK = (8, 12, 20)                                 # quant_per_token_cached behind the wave kernel (NV = 1, 2, 4, 6: unreachable)
OFF_BLOCK = (8, 20)                                    # quant_rows_off behind the wave kernel (NV = 1, 2, 4: unreachable)
NORM = (1, 2, 4, 8)                                    # norm_quant_cached, rmsnorm_rows
SILU = (2, 4, 6, 8)                                    # silu_mul_quant_cached, silu_mul_quant_fp8_cached

WAVE_PT_TOP = 64 * 28                                  # the wave kernels take per-token rows up to here (K / VEC) ...
WAVE_TENSOR_TOP = 64 * 24                              # ... and per-tensor image rows up to here
PT_BLOCK_TOP = 256 * 20                                # beyond: quant_per_token_generic
OFF_LIMIT = 256 * 20                                   # asq_quantize_act_off refuses longer rows
ROW_LIMIT = 256 * 8                                    # the norm / SiLU entries refuse longer rows


def ladder(tiers, lanes, max_nvec, lo=0):
    """K / VEC values: for each tier T of a `lanes`-wide ladder its top (lanes * T), one vector above it and one with a partial last round of 64 lanes"""
    out = []
    for t in tiers:
        for nvec in (lanes * (t - 1) + (27 if lanes == 64 else 91), lanes * t, lanes * t + 1):
            if lo < nvec <= max_nvec and nvec not in out:
                out.append(nvec)
    return out


def per_token_nvecs():
    """asq_quantize_act, per-token: the wave ladder, then quant_per_token_cached<8, 12, 20>; the last value (5121) is the generic kernel's"""
    return ladder(WAVE_I8, 64, WAVE_PT_TOP + 1) + ladder(PT_BLOCK, 256, PT_BLOCK_TOP + 1, lo=WAVE_PT_TOP + 1)


def off_nvecs(per_token):
    """asq_quantize_act_off: the wave ladder (per-tensor rows: up to 24 vectors per lane, per-token 28), then quant_rows_off<8, 20>"""
    top = WAVE_PT_TOP if per_token else WAVE_TENSOR_TOP
    return ladder(WAVE_I8, 64, top + 1) + ladder(OFF_BLOCK, 256, OFF_LIMIT, lo=top + 1)


def norm_nvecs():
    return ladder(NORM, 256, ROW_LIMIT)


def silu_nvecs():
    return ladder(SILU, 256, ROW_LIMIT)


def fp8_nvecs():
    """asq_quantize_act_fp8, per-token: the wave ladder; 1793 is the first row length of the block-per-row kernel"""
    return ladder(WAVE_F8, 64, WAVE_PT_TOP + 1)


# =====================================================================================================================================
# inputs
# =====================================================================================================================================
M_ROWS = 6            # the second 4-row block of the wave kernels is left half empty
#                  scale of the bulk   (the planted element is PLANT times the largest bulk magnitude of its row)
KINDS = {"x": 48.0,       # an activation: rounded per tensor, ~1 % of it clamps at +-127 and ~1 % rounds to 0
         "res": 20.0,     # the residual stream an "x" is added to (planted at the same places with the same signs)
         "acc": 1.0e3,    # an int32 accumulator (dq_add_layernorm_q; the planted elements stay below fp16's 65504: the entry converts it to dt first)
         "gate": 4.0,     # SiLU's gate: planted elements are POSITIVE (silu(-large) is 0), the sign of the product is `up`'s
         "up": 4.0}
PLANT = 8.0
SATURATING_GATES = (0.0, -0.0, 30.0, -30.0, 88.0, -100.0)      # the saturating branches of exp_det (tests/test_hip_n1.py)


def planted_columns(nvec, vec):
    """(r0, r1, r3, r4): element K - 1; the first element of the last vector; the first element of the last 64-lane round; of the last 256-thread round"""
    K = nvec * vec
    return K - 1, K - vec, vec * 64 * ((nvec + 63) // 64 - 1), vec * 256 * ((nvec + 255) // 256 - 1)


def rows(kind, dt, nvec, lanes, seed):
    """M_ROWS rows of nvec * VEC[dt] detrng values, rounded to dt (float32 array holding dt values; "acc": integers).
      r0  planted at element K - 1                 r1  planted, negative, at K - VEC (the first element of the last vector)
      r2  all zeros                                r3  planted at the first element of the last 64-lane round
      r4  planted at the first element of the last 256-thread round
      r5  the whole last vector same-signed and above everything else in the row: a duplicated or dropped last vector moves the mean, the variance,
          the absolute maximum and row_off's sum
    A planted element is PLANT times the largest magnitude of the rest of its row.  `lanes` (64 | 256) is the width of the ladder nvec comes from: it
    selects the random stream only, the planted places cover both widths whatever it is."""
    assert kind in KINDS and lanes in (64, 256) and nvec >= 1
    vec = VEC[dt]
    K = nvec * vec
    stream = (nvec * 8 + list(KINDS).index(kind)) * 2 + (lanes == 256)
    x = detrng.normal(seed, stream, (M_ROWS, K)).astype(np.float64) * KINDS[kind]
    c0, c1, c3, c4 = planted_columns(nvec, vec)
    sign1 = 1.0 if kind == "gate" else -1.0
    for r, c, sg in ((0, c0, 1.0), (1, c1, sign1), (3, c3, 1.0), (4, c4, 1.0)):
        x[r, c] = 0.0
        x[r, c] = sg * PLANT * max(np.abs(x[r]).max(), KINDS[kind])
    x[2] = 0.0
    top = max(np.abs(x[5, :K - vec]).max(initial=0.0), KINDS[kind])
    x[5, K - vec:] = 1.25 * top * (1.0 - 0.02 * np.arange(vec))
    if kind == "acc":
        return np.rint(x).astype(np.float32)
    return O.round_to(x.astype(np.float32), dt)


def norm_params(dt, K, seed):
    """(weight, bias) of a scale-folded norm: weight ~ 1 / 0.04 (y = weight * normalised x is rounded per tensor: some of it clamps, some rounds to 0)"""
    w = (detrng.normal(seed, 900001, (K,)) * np.float32(0.1) + np.float32(1.0)) / np.float32(0.04)
    b = detrng.normal(seed, 900002, (K,)) * np.float32(3.0)
    return O.round_to(w.astype(np.float32), dt), O.round_to(b.astype(np.float32), dt)


def silu_rows(dt, nvec, seed):
    """(gate, up) whose product carries the planted places of rows(); r0 starts with the saturating gates"""
    g, u = rows("gate", dt, nvec, 256, seed), rows("up", dt, nvec, 256, seed)
    g[0, :len(SATURATING_GATES)] = O.round_to(np.array(SATURATING_GATES, np.float32), dt)
    return g, u


def dq_add_h(acc, res, dt, scale, once=False):
    """asq_dq_add_layernorm_q's residual output, torch.add(res, acc.to(dt), alpha=scale): h = dt(f32(fma(scale, f32(dt(acc)), f32(res)))) -- ONE fp32 multiply-add,
    then the rounding to dt (include/asq_hip.h).  once=True: the exact sum rounded to dt directly, which is what a fused fp16 multiply-add instruction returns.
    float64 holds the product (24 x <= 24 bits) and, for the magnitudes rows() makes, the sum exactly: asserted."""
    a = O.round_to(np.asarray(acc, np.float32), dt).astype(np.float64)
    r = np.asarray(res, np.float32).astype(np.float64)
    p = np.float64(np.float32(scale)) * a
    t = p + r
    assert np.array_equal((t - p) - r, np.zeros_like(t)) and np.array_equal((t - r) - p, np.zeros_like(t)), "the float64 sum is not exact"
    if not once:
        return O.round_to(t.astype(np.float32), dt)
    if dt == "f16":
        return t.astype(np.float16).astype(np.float32)
    if dt == "f32":
        return t.astype(np.float32)
    f = t.astype(np.float32)                          # bf16 from float64 in one rounding: round to odd into fp32 (16 spare bits), then to nearest even
    exact = f.astype(np.float64) == t
    other = np.nextafter(f, np.where(f.astype(np.float64) > t, np.float32(-np.inf), np.float32(np.inf)))
    odd = np.where((f.view(np.uint32) & 1) == 1, f, other)
    return O.round_to(np.where(exact, f, odd).astype(np.float32), dt)


def drop_last_vector(x, dt):
    y = x.copy()
    y[:, -VEC[dt]:] = 0
    return y


def repeat_last_vector(x, dt):
    return np.concatenate([x, x[:, -VEC[dt]:]], axis=1)


def first_difference(got, want):
    """None when the two arrays hold the same bytes, else 'row r: n elements differ, first at i (got .. want ..), last at j'"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"shape / dtype {got.shape} {got.dtype} != {want.shape} {want.dtype}"
    g2, w2 = got.reshape(got.shape[0], -1) if got.ndim else got.reshape(1, 1), want.reshape(want.shape[0], -1) if want.ndim else want.reshape(1, 1)
    gb = np.ascontiguousarray(g2).view(np.uint8).reshape(g2.shape[0], g2.shape[1], -1)
    wb = np.ascontiguousarray(w2).view(np.uint8).reshape(gb.shape)
    bad = (gb != wb).any(axis=2)
    if not bad.any():
        return None
    r = int(np.nonzero(bad.any(axis=1))[0][0])
    idx = np.nonzero(bad[r])[0]
    return (f"{int(bad.sum())} elements in {int(bad.any(axis=1).sum())} rows differ; row {r}: {idx.size} differ, first at {int(idx[0])} (got {g2[r, idx[0]]!r}, want "
            f"{w2[r, idx[0]]!r}), last at {int(idx[-1])} (got {g2[r, idx[-1]]!r}, want {w2[r, idx[-1]]!r})")


# =====================================================================================================================================
# whole-domain rows of the per-token quotient (RowDivisor / QRowFast: Markstein's sequence, with a switch to the plain division)
# =====================================================================================================================================
WD_ROW = 4096        # elements per row, before the vector that pins the row maximum


def _prev(v, dt):
    """the largest dt value below the positive dt value v"""
    v = np.float32(v)
    if dt == "f32":
        return np.nextafter(v, np.float32(0))
    if dt == "f16":
        return np.float32(np.nextafter(np.float16(v), np.float16(0)))
    return (np.array([v], np.float32).view(np.uint32) - np.uint32(0x10000)).view(np.float32)[0]


def _ceil_dt(v, dt):
    """the smallest dt value >= v (v positive, in range)"""
    r = O.round_to(np.array([v], np.float32), dt)[0]
    if r >= np.float32(v):
        return r
    if dt == "f32":
        return np.nextafter(r, np.float32(np.inf))
    return (np.array([r], np.float32).view(np.uint32) + np.uint32(0x10000)).view(np.float32)[0]       # (bf16 only: no fp16 case asks for it)


def whole_domain_maxima(dt):
    """{id: row maximum m}: every case quantises values |x| <= m in rows that all hold +m and -m (so every row has the scale dt(m / 127))"""
    big = {"f16": 65504.0, "bf16": float(np.array([0x7F7F0000], np.uint32).view(np.float32)[0]), "f32": float(np.finfo(np.float32).max)}[dt]
    out = {f"127x2^{e}": 127.0 * 2.0 ** e for e in (-14, -3, 0, 5)}       # the scale is exactly 2^e: every half-integer quotient occurs
    out["1.0"] = 1.0
    out["largest"] = big
    if dt == "f16":
        out["2^-20"] = 2.0 ** -20                                         # a non-zero row whose scale rounds to 0: +-inf and NaN quotients
    else:
        for e in (60, 59, -60, -59):                                      # the scale is 2^e: either side of the fast path's 2^-60 < s < 2^60
            out[f"127x2^{e}"] = 127.0 * 2.0 ** e
        at = _ceil_dt(3.0e38, dt)                                          # the fast path asks for a row maximum < 3.0e38f
        out[">=3e38"] = float(at)
        out["<3e38"] = float(_prev(at, dt))
    return out


def _all_16bit(dt):
    bits = np.arange(65536, dtype=np.uint32)
    if dt == "f16":
        return bits.astype(np.uint16).view(np.float16).astype(np.float32)
    return (bits << 16).astype(np.uint32).view(np.float32).copy()


def _neighbours(v, dt):
    """v (dt values) and both neighbours of each in dt"""
    v = np.asarray(v, np.float32)
    if dt == "f32":
        return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])
    if dt == "f16":
        h = v.astype(np.float16)
        return np.concatenate([h, np.nextafter(h, np.float16(-np.inf)), np.nextafter(h, np.float16(np.inf))]).astype(np.float32)
    u = v.view(np.uint32).astype(np.int64)
    mag, neg = u & 0x7FFFFFFF, (u >> 31) & 1
    up = np.where(neg == 1, np.where(mag == 0, 0x00010000, (mag - 0x10000) | 0x80000000), mag + 0x10000)        # towards +inf
    dn = np.where(neg == 0, np.where(mag == 0, 0x80010000, mag - 0x10000), (mag + 0x10000) | 0x80000000)        # towards -inf
    return np.concatenate([v, up.astype(np.uint32).view(np.float32), dn.astype(np.uint32).view(np.float32)])


def half_integer_points(dt, m):
    """dt((k + 0.5) * s) for k in [-128, 127] and s = dt(m / 127), with both neighbours of each in dt: where a mis-rounded quotient changes the int8"""
    s = np.float64(O.round_to(np.array([np.float32(m) / np.float32(127.0)], np.float32), dt)[0])
    with np.errstate(over="ignore", invalid="ignore"):
        c = O.round_to(((np.arange(-128, 128) + 0.5) * s).astype(np.float32), dt)
        return _neighbours(c, dt)


def whole_domain_values(dt, m, seed=77):
    """1-D float32 array of dt values, all finite with |x| <= m.
    fp16 / bf16: EVERY such bit pattern (which includes half_integer_points).
    fp32: (k + 0.5) * s * (1 + j * 2^-23) for k in [-128, 127], j in -2 .. 2; half_integer_points; 4096 random patterns with |x| <= m."""
    m = np.float32(m)
    if dt != "f32":
        v = _all_16bit(dt)
    else:
        s = np.float64(np.float32(m) / np.float32(127.0))
        k, j = np.meshgrid(np.arange(-128, 128) + 0.5, np.arange(-2, 3), indexing="ij")
        with np.errstate(over="ignore"):
            grid = (k * s * (1.0 + j * 2.0 ** -23)).astype(np.float32).reshape(-1)
        u = detrng.u64(seed, 1, 4096)
        frac = (u & np.uint64(0x7FFFFF)).astype(np.uint32)
        sign = ((u >> np.uint64(23)) & np.uint64(1)).astype(np.uint32)
        etop = int(np.array([m], np.float32).view(np.uint32)[0] >> 23)
        expo = ((u >> np.uint64(24)) % np.uint64(etop + 1)).astype(np.uint32)
        rnd = ((sign << 31) | (expo << 23) | frac).view(np.float32)
        v = np.concatenate([grid, half_integer_points(dt, m), rnd])
    with np.errstate(invalid="ignore"):
        return v[np.isfinite(v) & (np.abs(v) <= m)].astype(np.float32)


def whole_domain_rows(dt, m):
    """whole_domain_values in rows of WD_ROW (the last one zero-padded), each followed by one vector {+m, -m, 0 ..}: [R, WD_ROW + VEC]"""
    v = whole_domain_values(dt, m)
    R = (v.size + WD_ROW - 1) // WD_ROW
    body = np.zeros(R * WD_ROW, np.float32)
    body[:v.size] = v
    x = np.zeros((R, WD_ROW + VEC[dt]), np.float32)
    x[:, :WD_ROW] = body.reshape(R, WD_ROW)
    x[:, WD_ROW], x[:, WD_ROW + 1] = np.float32(m), -np.float32(m)
    return x


def exact_half_integer_quotients(x, dt):
    """the number of DISTINCT values in x (whole_domain_rows: one scale for all rows) whose exact quotient by the oracle's scale dt(max|x| / 127) is k + 0.5
    with |quotient| < 128"""
    m = np.abs(x).max()
    s = np.float64(O.round_to(np.array([np.float32(m) / np.float32(127.0)], np.float32), dt)[0])
    if s == 0:
        return 0
    q = np.unique(x.astype(np.float64)) / s          # exact for a power-of-two s
    return int(((np.abs(q) < 128) & (np.floor(q) + 0.5 == q)).sum())


def is_power_of_two(s):
    return s > 0 and (int(np.array([s], np.float32).view(np.uint32)[0]) & 0x7FFFFF) == 0 and np.isfinite(s)
