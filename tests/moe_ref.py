"""numpy restatements of the three rules of include/asq_hip_moe.h: the yardstick of tests/test_hip_moe_*.py, checked itself in tests/test_moe_cpu.py.

route(logits, top_k, w_dtype)
    Selection: on the logits as fp32, descending; ties (-0 == +0) to the lower expert index; a NaN ranks below every number, NaNs among themselves by index.
    Weights: m = the first selected logit, e_j = expf(l_j - m), w_j = e_j / (e_0 + ... + e_{k-1}) summed in fp32 in slot order, rounded once to w_dtype -- `w32`
    is that fp32 sequence with numpy's expf, `w64` the same expression in float64 (the exact weights of the fp32 logits to ~1e-16): the GPU tests bound the
    library's weights against w64, since two correct expf implementations need not agree in the last place.
    Order: a stable counting sort of the pairs (t, j) by expert -- tok = argsort(sel.flatten(), stable) // top_k, group_offsets = cat(0, cumsum(bincount)),
    inv[t, j] = the sorted row of pair (t, j).
combine(y, wts, inv, dt)
    acc_0 = 0, acc_{j+1} = fp32(acc_j + fp32(y[inv[t, j]] * wts[t, j])), one rounding to dt."""
import numpy as np

DTS = ("f32", "f16", "bf16")
SIG = {"f32": 24, "f16": 11, "bf16": 8}        # significand bits
MID_REL = 2.0 ** -20                           # a weight this close (relative) to a rounding midpoint of dt may round either way


def bf16_round(x32):
    """fp32 -> the nearest bf16 value (RNE), as fp32; NaN stays NaN"""
    x32 = np.ascontiguousarray(x32, np.float32)
    u = x32.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16).astype(np.uint32)
    return np.where(np.isnan(x32), np.float32(np.nan), r.view(np.float32))


def round_f32_to(x32, dt):
    """one RNE rounding of fp32 values to dt, returned as fp32"""
    x32 = np.asarray(x32, np.float32)
    if dt == "f32":
        return x32
    with np.errstate(over="ignore"):
        return x32.astype(np.float16).astype(np.float32) if dt == "f16" else bf16_round(x32)


def round_f64_to(x, dt):
    """one RNE rounding of POSITIVE NORMAL float64 values straight to dt (no double rounding through fp32), as float64"""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                         # x = m * 2^e, 0.5 <= m < 1
    p = SIG[dt]
    return np.ldexp(np.rint(m * 2.0 ** p), e - p)


def ulp_of(x, dt):
    """the spacing of dt at positive normal x"""
    _, e = np.frexp(np.asarray(x, np.float64))
    return np.ldexp(1.0, e - SIG[dt])


def near_midpoint(x, dt, rel=MID_REL):
    """True where positive x lies within rel * x of the midpoint between two neighbouring dt values"""
    x = np.asarray(x, np.float64)
    m, _ = np.frexp(x)
    q = m * 2.0 ** SIG[dt]
    return np.abs(q - np.floor(q) - 0.5) <= rel * q


def select(logits, top_k):
    """sel int32 [T, k]: the rule's order, best first"""
    l = np.asarray(logits, np.float32)
    T, E = l.shape
    nan = np.isnan(l)
    v = np.where(nan, np.float32(0), l)
    idx = np.broadcast_to(np.arange(E), (T, E))
    order = np.lexsort((idx, -v, nan), axis=-1)       # primary: numbers before NaNs; then descending value (-0.0 == 0.0); then the index
    return order[:, :top_k].astype(np.int32)


def weights(logits, sel, w_dtype="f32"):
    """(w of w_dtype as fp32 from the fp32 sequence, w64): [T, k] each"""
    l = np.asarray(logits, np.float32)
    ls = np.take_along_axis(l, sel.astype(np.int64), axis=1)
    with np.errstate(all="ignore"):
        e32 = np.exp((ls - ls[:, :1]).astype(np.float32)).astype(np.float32)
        d = e32[:, 0].copy()
        for j in range(1, sel.shape[1]):
            d = (d + e32[:, j]).astype(np.float32)
        w32 = (e32 / d[:, None]).astype(np.float32)
        e64 = np.exp(ls.astype(np.float64) - ls[:, :1].astype(np.float64))
        d64 = e64[:, 0].copy()
        for j in range(1, sel.shape[1]):
            d64 = d64 + e64[:, j]
        w64 = e64 / d64[:, None]
    return round_f32_to(w32, w_dtype), w64


def sort_pairs(sel, E):
    """(group_offsets int32 [E + 1], tok int32 [T * k], inv int32 [T, k]) of the stable sort of the pairs by expert"""
    T, k = sel.shape
    flat = sel.reshape(-1)
    order = np.argsort(flat, kind="stable")
    offs = np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]).astype(np.int32)
    inv = np.empty(T * k, np.int32)
    inv[order] = np.arange(T * k, dtype=np.int32)
    return offs, (order // k).astype(np.int32), inv.reshape(T, k)


def route(logits, top_k, w_dtype="f32"):
    """dict(sel, wts, w64, group_offsets, tok, inv)"""
    sel = select(logits, top_k)
    w, w64 = weights(logits, sel, w_dtype)
    offs, tok, inv = sort_pairs(sel, np.asarray(logits).shape[1])
    return {"sel": sel, "wts": w, "w64": w64, "group_offsets": offs, "tok": tok, "inv": inv}


def check_safety(sel, offs, tok, inv, T, E, k):
    """the safety property, whatever the logits held"""
    assert sel.shape == (T, k) and (sel >= 0).all() and (sel < E).all()
    assert all(len(set(r)) == k for r in sel.tolist()), "a token's experts are not distinct"
    assert offs[0] == 0 and offs[-1] == T * k and (np.diff(offs) >= 0).all()
    assert np.array_equal(np.sort(inv.reshape(-1)), np.arange(T * k)), "inv is no permutation"
    assert np.array_equal(tok[inv.reshape(-1)], np.repeat(np.arange(T), k)), "tok[inv[t, j]] != t"
    rows_expert = np.repeat(np.arange(E), np.diff(offs))
    assert np.array_equal(rows_expert[inv.reshape(-1)], sel.reshape(-1)), "a pair's row lies outside its expert's group"


def combine(y, wts, inv, dt):
    """y [R, H] (values of dt as fp32), wts fp32 [T, k], inv [T, k] -> out [T, H] of dt as fp32: the fp32 sequence, one rounding"""
    y, wts = np.asarray(y, np.float32), np.asarray(wts, np.float32)
    acc = np.zeros((inv.shape[0], y.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for j in range(inv.shape[1]):
            acc = (acc + (y[inv[:, j]] * wts[:, j, None]).astype(np.float32)).astype(np.float32)
    return round_f32_to(acc, dt)


def combine64(y, wts, inv):
    """the same sum in float64"""
    y, wts = np.asarray(y, np.float64), np.asarray(wts, np.float64)
    return sum(y[inv[:, j]] * wts[:, j, None] for j in range(inv.shape[1]))


def gapped_logits(T, E, seed, spread=8.0, dt="f32"):
    """[T, E] fp32 logits representable in dt, every row a shuffled ladder of E distinct values at least spread / (2 E) apart inside a range of `spread`: the top-k
    (and top-(k+1)) values of a row are distinct in every dtype, and a softmax over them in fp32 cannot reorder them"""
    rng = np.random.default_rng(seed)
    step = spread / max(E, 2)
    base = (np.arange(E) * step)[None, :] + rng.uniform(0, step / 2, (T, E))
    l = np.take_along_axis(base, rng.permuted(np.broadcast_to(np.arange(E), (T, E)), axis=1), axis=1)
    l = l - spread / 2 + rng.uniform(-0.25, 0.25, (T, 1))
    return np.ascontiguousarray(round_f32_to(l.astype(np.float32), dt))
