"""Adversarial operands for asq_bmm_i8's softmax kinds (bmm_i8_sm128), their expected values, and an fp32 emulation of the kernel's two-pass online softmax with
arithmetic mutants.  Shared by tests/test_softmax_adversarial_cpu.py (no GPU) and tests/test_hip_bmm_softmax_adversarial.py (-m gpu) so that both see the same
inputs.  No device, no test functions in here.  The acceptance rule is softmax_q8_ref's target / judge / check with its own BAND_CAP; nothing is added to it.

Why: with uniform random operands the scores of a row are i.i.d., so the running reference of the online softmax is found in the first tile or two, keys hidden by
the causal mask score like visible ones, and an error of the offset o cancels between a row's numerators and its sum.  The operands here order the scores instead:

  keys     key n holds bytes whose sum is level(n), spread over all K positions and permuted; a query of +-127 everywhere gives acc[m, n] = +-127 level(n), monotone
           in n for every row (keys_from_levels, ramp_levels, queries).
  hard     (family b) alpha puts neighbouring keys >= 100 nats apart: a row is one-hot on the best key it sees -- 127 at n = m + N - M under the causal mask, at
           N - 1 without it, at 0 for a -127 query -- byte-exact, no band.  Every tile moves the reference, every rescale and every losing slot of the merge underflows
           to 0, every future key leads every visible one, and a key limit off by one either way moves every row.  With ties: the g best keys equal, rne(127 / g) each.
  soft     (family c) the same keys at about 0.45 nats (and 3 nats) per key, in every order of ORDERS; band rule.
  place    (family d) the orders that put the row maximum on column 0, on a tile seam, in the partial last tile, and in one merge slot only (slot_case).
  range    (family e) the hard staircase at alpha 1, -1 and 1e3 (|alpha acc| up to 1e9), alpha of no effect (1e-30, a denormal, +-0), accumulators beyond 2^24.

emulate() restates the kernel (csrc/asq_bmm.hip, bmm_i8_sm128) in fp32 numpy: 128-row blocks, 128-column tiles, the eight (wave column, lane quarter) slots of a row
with their own reference / o / l, merged in slot order, pass 2 from the merged o.  MUTANTS are the faults the families are there to see; the CPU test asserts which
family rejects which (EXPECTED_TABLE)."""
import functools

import numpy as np

import softmax_q8_ref as R

F32, F64 = np.float32, np.float64
SEED = 8128
TILE = 128
NATS_HARD = 100.0          # neighbouring levels of the hard staircase are at least this far apart
NATS_FAR = 150.0           # what "out of reach" means for the slot cases: exp(-150) * 2^24 is far below fp32's smallest normal times any l

# (M, N, K): K = 16, 128 keep the A tile in LDS, 144 and 272 reload it every tile (2 and 3 K steps), 33 takes the byte path
HARD_SHAPES = [(300, 300, 128), (140, 300, 64), (300, 140, 144), (130, 257, 33), (16, 300, 128), (1, 257, 16), (257, 129, 272)]
TIES = (3, 4, 5)           # 2 and 254 would be ties of the rounding (63.5, 0.5)
TIE_SHAPES = [(300, 300, 128), (130, 257, 33), (140, 300, 64)]
SOFT_SHAPES = [(300, 300, 128), (140, 300, 64), (130, 257, 33)]
SOFT_NATS = (0.45, 3.0)
RANGE_SHAPES = [(140, 300, 64), (130, 257, 33), (1, 257, 16)]      # 127 * 127 * 64 * 1e3 = 1.03e9
RANGE_ALPHAS = (1.0, -1.0, 1e3)
NULL_ALPHAS = (1e-30, 1e-40, -0.0, 0.0)                            # 1e-40 is a denormal in fp32
BIG_SHAPE = (20, 140, 2048)
BATCHES = (1, 3)


def ident(shape):
    return "x".join(map(str, shape))


def _rng(*key):
    return np.random.default_rng([SEED, *[int(k) for k in key]])


def _frozen(*arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# keys and queries
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def hard_alpha(K):
    """the alpha of the hard staircase: neighbouring ramp levels >= NATS_HARD apart at the shapes above (the CPU test re-derives it)"""
    return 0.01 if K >= 128 else 0.02 if K >= 64 else 0.05 if K >= 33 else 0.1


def level_gap(N, K, extra=0):
    """the largest integer gap g with (N - 1 + extra) g <= 255 K: N (+ extra) levels g apart fit [-128 K, 127 K]"""
    g = (255 * K) // max(N - 1 + extra, 1)
    assert g >= 1, (N, K, extra)
    return g


def ramp_levels(N, K, tie=0):
    """strictly ascending levels over [-128 K, 127 K], the top at 127 K.  tie = g > 1: runs of g equal levels, aligned to the END (the g best keys are equal; the
    first run may be shorter)"""
    if tie > 1:
        run = (N - 1 - np.arange(N)) // tie                      # 0 for the last g keys
        g = level_gap(int(run.max()) + 1, K)
        return 127 * K - g * run
    g = level_gap(N, K)
    return 127 * K - g * (N - 1 - np.arange(N))


def keys_from_levels(levels, K, *seed):
    """int8 [N, K]: row n sums to levels[n]; floor(level / K) everywhere, +1 on level mod K positions, the positions permuted per key"""
    levels = np.asarray(levels, np.int64)
    assert levels.min() >= -128 * K and levels.max() <= 127 * K
    base, rem = np.divmod(levels, K)
    vals = base[:, None] + (np.arange(K)[None, :] < rem[:, None])
    perm = np.argsort(_rng(*seed, 1).random(vals.shape), axis=1)
    b = np.take_along_axis(vals, perm, axis=1)
    assert b.min() >= -128 and b.max() <= 127 and np.array_equal(b.sum(1), levels)
    return b.astype(np.int8)


def ramp_keys(N, K, *seed):
    return keys_from_levels(ramp_levels(N, K), K, *seed)


def row_signs(M, entry, *seed):
    """entry 0: every query +127 (ascending scores); entry 1: every query -127 (descending); entry 2 and on: a seeded mix"""
    if entry % 3 == 0:
        return np.ones(M, np.int64)
    if entry % 3 == 1:
        return -np.ones(M, np.int64)
    return np.where(_rng(*seed, entry, 2).random(M) < 0.5, 1, -1).astype(np.int64)


def queries(signs, K):
    return np.repeat((127 * signs).astype(np.int8)[:, None], K, axis=1)


def one_hot(levels, signs, M, N, causal, negative_alpha=False):
    """the by-design bytes of a row whose best visible level leads by >= NATS_HARD nats: rne(127 / r) on the r keys that share it, 0 elsewhere, all zero without
    a visible key.  -> (want int8 [M, N], half [M] bool: rows with r = 2, where 63.5 may round either way and the two bytes are compared as {63, 64})"""
    vis = R.visible(M, N, causal)
    eff = signs * (-1 if negative_alpha else 1)
    s = eff[:, None] * np.asarray(levels, np.int64)[None, :]
    s = np.where(vis, s, np.iinfo(np.int64).min)
    top = vis & (s == s.max(axis=1, keepdims=True))
    r = top.sum(1)
    want = np.where(top, np.rint(127.0 / np.maximum(r, 1))[:, None], 0).astype(np.int8)
    return want, r == 2


def check_one_hot(q, want, half, what=""):
    """byte-exact; on a row with two equal leaders the two bytes are 63 or 64 (t = 63.5 exactly: softmax_q8_ref's tie) and the rest exact"""
    q = np.asarray(q)
    assert q.shape == want.shape, (q.shape, want.shape)
    ok = q == want
    tie = (want == 64) & half[..., None]
    ok |= tie & (q == 63)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} bytes differ from the staircase in {len(set(map(tuple, bad[:, :-1])))} rows, first at {i}: got {q[i]}, want {want[i]}")


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# family b / e: the hard staircase
# ---------------------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hard_operands(shape, entries, tie=0):
    """-> a int8 [entries, M, K], b int8 [entries, N, K], levels [entries, N], signs [entries, M]: per entry its own byte spread and sign pattern (row_signs)"""
    M, N, K = shape
    levels = np.stack([ramp_levels(N, K, tie) for _ in range(entries)])
    b = np.stack([keys_from_levels(levels[i], K, M, N, K, tie, i) for i in range(entries)])
    signs = np.stack([row_signs(M, i, M, N, K, tie) for i in range(entries)])
    a = np.stack([queries(signs[i], K) for i in range(entries)])
    return _frozen(a, b, levels, signs)


def hard_want(shape, levels, signs, causal, negative_alpha=False):
    """-> (want [entries, M, N], half [entries, M]) of hard_operands' levels and signs"""
    M, N, _ = shape
    pairs = [one_hot(levels[i], signs[i], M, N, causal, negative_alpha) for i in range(len(levels))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


@functools.lru_cache(maxsize=None)
def head_operands(shape, S, h, r, ties):
    """The staircase for the grouped and token-major forms: S sequences of h query heads over h / r key heads, head-major.
    -> a int8 [S * h, M, K], b int8 [S * h / r, N, K], levels [S * h / r, N], signs [S * h, M].  Every key head has its own bytes and (ties) its own run length
    of equal levels, 1, 3, 4, 5 in turn; query head e meets key head e // r and carries row_signs(M, e): the r heads of a group differ in sign."""
    M, N, K = shape
    nb = S * h // r
    assert nb * r == S * h
    levels = np.stack([ramp_levels(N, K, (0, 3, 4, 5)[j % 4] if ties else 0) for j in range(nb)])
    b = np.stack([keys_from_levels(levels[j], K, M, N, K, S, h, r, j) for j in range(nb)])
    signs = np.stack([row_signs(M, e, M, N, K, S, h, r) for e in range(S * h)])
    a = np.stack([queries(s, K) for s in signs])
    return _frozen(a, b, levels, signs)


def head_want(shape, levels, signs, r, causal):
    """-> (want [S * h, M, N], half [S * h, M]) of head_operands' levels and signs"""
    return hard_want(shape, levels[np.arange(len(signs)) // r], signs, causal)


# (S, h, r) of the kernel forms: plain, GROUPED with r = 4 and 8, TOKEN without and with a group
FORMS = {"plain": (3, 1, 1), "group4": (1, 8, 4), "group8": (1, 8, 8), "token": (2, 3, 1), "token-group2": (2, 4, 2)}
FORM_SHAPES = {"k64": (140, 300, 64), "k33": (140, 300, 33)}       # K % 16 == 0: FAST when the operands are aligned; 33: the byte path


def min_gap_nats(levels, alpha):
    """the smallest distance in nats between two different scores +-127 level * alpha"""
    d = np.diff(np.unique(levels))
    return float(127.0 * abs(F64(F32(alpha))) * d.min()) if d.size else np.inf


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# families c / d: the soft ramp in every order
# ---------------------------------------------------------------------------------------------------------------------------------------------------
ORDERS = ("asc", "desc", "max0", "max127", "max128", "maxlast", "saw-up", "saw-down")


def order_of(name, N, *seed):
    """src [N]: column j holds the key of rank src[j] (rank 0 the lowest level).  asc is the causal rows' "maximum on my own last visible column"; max<c> shuffles
    the keys and puts the best one on column c (maxlast: N - 1, in the partial last tile); saw-up ascends inside every 128-tile and descends across tiles (the
    first tile holds the best keys), saw-down is its mirror."""
    idx = np.arange(N)
    if name == "asc":
        return idx
    if name == "desc":
        return idx[::-1].copy()
    if name.startswith("max"):
        col = {"max0": 0, "max127": 127, "max128": 128, "maxlast": N - 1}[name]
        assert col < N
        src = _rng(*seed, 3).permutation(N)
        at = int(np.flatnonzero(src == N - 1)[0])
        src[at], src[col] = src[col], src[at]
        return src
    tile, pos = idx // TILE, idx % TILE
    size = np.minimum(TILE, N - tile * TILE)
    if name == "saw-up":
        return N - tile * TILE - size + pos
    if name == "saw-down":
        return tile * TILE + size - 1 - pos
    raise ValueError(name)


def soft_alpha(N, K, nats, extra=0):
    return float(F32(nats / (127.0 * level_gap(N, K, extra))))


@functools.lru_cache(maxsize=None)
def soft_operands(shape, entries, order):
    """-> a [entries, M, K], b [entries, N, K], src [entries, N]: ramp_keys in the given order, per entry its own bytes, shuffle and signs"""
    M, N, K = shape
    src = np.stack([order_of(order, N, M, N, K, i) for i in range(entries)])
    b = np.stack([ramp_keys(N, K, M, N, K, 50 + i)[src[i]] for i in range(entries)])
    a = np.stack([queries(row_signs(M, i, M, N, K, 50), K) for i in range(entries)])
    return _frozen(a, b, src)


def slot_columns(N, slot):
    """the columns whose scores the merge slot `slot` = wn * 4 + q16 holds: column 64 wn + 16 j + 4 q16 + e of every tile"""
    c = np.arange(N) % TILE
    return np.flatnonzero((c // 64) * 4 + (c % 16) // 4 == slot)


@functools.lru_cache(maxsize=None)
def slot_case(shape, entries, slot):
    """-> a, b, alpha: a soft ramp (0.45 nats per key) on the columns of one merge slot, shuffled; every other column lower by >= NATS_FAR nats plus its own ramp.
    Queries +127: the seven other partials of a row lose the merge outright (lp * exp2(orow - o_p) underflows to 0)."""
    M, N, K = shape
    far = int(np.ceil(NATS_FAR / 0.45))
    g = level_gap(N, K, far)
    cols = slot_columns(N, slot)
    rest = np.setdiff1d(np.arange(N), cols)
    bs = []
    for i in range(entries):
        rng = _rng(M, N, K, slot, i, 4)
        rank = np.empty(N, np.int64)                              # 0 = the top
        rank[cols] = rng.permutation(len(cols))
        rank[rest] = len(cols) + far + rng.permutation(len(rest))
        bs.append(keys_from_levels(127 * K - g * rank, K, M, N, K, slot, i))
    a = np.repeat(queries(np.ones(M, np.int64), K)[None], entries, 0)
    return _frozen(a, np.stack(bs)) + (soft_alpha(N, K, 0.45, far),)


def slots_without_a_key(M, N):
    """[M, tiles, 8] bool under the causal mask: the row sees keys of the tile, but none of this slot's"""
    vis = R.visible(M, N, True)
    nt = -(-N // TILE)
    out = np.zeros((M, nt, 8), bool)
    for t in range(nt):
        sees = vis[:, t * TILE:(t + 1) * TILE].any(1)
        for s in range(8):
            cols = slot_columns(N, s)
            cols = cols[cols // TILE == t]
            out[:, t, s] = sees & ~vis[:, cols].any(1)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# family e: accumulators beyond 2^24
# ---------------------------------------------------------------------------------------------------------------------------------------------------
BIG_ALPHA = 1.5e-6


@functools.lru_cache(maxsize=None)
def big_operands(entries):
    """M = 20, N = 140, K = 2048.  Queries of -128 everywhere, so acc = -128 sum(b).  Three groups of keys: all -128 (acc = 2^25, the top), 32 of the positions
    +127 instead (255 * 2^12 lower), all +127 (255 * 2^18 lower).  Every accumulator is a multiple of 2^12, exact in fp32.  With BIG_ALPHA the groups lie 0, 1.57
    and 100.3 nats below the top.  Per entry 3 top and 5 second keys at seeded columns, at least one of each behind column 128 (the second tile, which the causal
    mask opens row by row)."""
    M, N, K = BIG_SHAPE
    bs = []
    for i in range(entries):
        rng = _rng(M, N, K, i, 5)
        cols = np.concatenate([rng.permutation(TILE)[:6], TILE + rng.permutation(N - TILE)[:2]])
        b = np.full((N, K), 127, np.int8)
        b[cols[[0, 1, 6]]] = -128
        for n in cols[[2, 3, 4, 5, 7]]:
            b[n] = -128
            b[n, rng.permutation(K)[:32]] = 127
        bs.append(b)
    a = np.full((entries, M, K), -128, np.int8)
    return _frozen(a, np.stack(bs))


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the kernel restated in fp32, and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------------------------
MUTANTS = ("max-over-masked", "sum-over-masked", "no-rescale", "rescale-sign", "limit+1", "limit-1", "merge-ignores-ref", "pass2-own-o")
LOG2E = F32(1.44269502162933349609375)
MAGIC = F64(12582912.0)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# column of (slot, element): slot = wn * 4 + q16, element = 4 j + e -> 64 wn + 16 j + 4 q16 + e
_SLOT_COLS = np.array([[64 * (s // 4) + 16 * j + 4 * (s % 4) + e for j in range(4) for e in range(4)] for s in range(8)])


def _exp2(x):
    """v_exp_f32: fp32 in, fp32 out, results below the smallest normal flushed to 0"""
    with np.errstate(all="ignore"):
        y = np.exp2(x.astype(F64)).astype(F32)
    return np.where(y < F32(2.0 ** -126), F32(0), y)


def _fma(x, y, z):
    with np.errstate(all="ignore"):
        return (np.asarray(x, F64) * np.asarray(y, F64) + np.asarray(z, F64)).astype(F32)


def _seq_sum(terms):
    """fp32 sum over the last axis, left to right"""
    s = np.zeros(terms.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for i in range(terms.shape[-1]):
            s = (s + terms[..., i]).astype(F32)
    return s


def emulate(acc, alpha, causal, mutant=None):
    """acc int [M, N] -> uint8 [M, N]: bmm_i8_sm128's arithmetic per row, tile and slot, as the kernel's comment states it.  mutant: one of MUTANTS or None"""
    assert mutant is None or mutant in MUTANTS, mutant
    acc = np.asarray(acc, np.int64)
    M, N = acc.shape
    alpha = F32(alpha)
    with np.errstate(all="ignore"):
        c = F32(alpha * LOG2E)
    neg = bool(alpha < 0)
    ref0 = INT32_MAX if neg else INT32_MIN
    best = (lambda x, y: np.minimum(x, y)) if neg else (lambda x, y: np.maximum(x, y))
    limit = np.full(M, N, np.int64)
    if causal:
        limit = np.arange(M) + (N - M) + 1 + {"limit+1": 1, "limit-1": -1}.get(mutant, 0)
    limit = np.clip(limit, 0, N)
    out = np.zeros((M, N), np.uint8)
    with np.errstate(all="ignore"):
        for m0 in range(0, M, TILE):
            rows = np.arange(m0, min(m0 + TILE, M))
            lim = limit[rows][:, None, None]
            nt = -(-int(limit[rows[-1]]) // TILE)
            ref = np.full((len(rows), 8), ref0, np.int64)
            l = np.zeros((len(rows), 8), F32)
            o = -(ref.astype(F32) * c)
            tiles = []
            for t in range(nt):
                cols = t * TILE + _SLOT_COLS                                          # [8, 16]
                a = acc[rows][:, np.minimum(cols, N - 1)]                            # [rows, 8, 16]
                vis = cols[None] < lim
                tiles.append((cols, a, vis))
                in_max = np.broadcast_to(cols[None] < N, vis.shape) if mutant == "max-over-masked" else vis
                in_sum = np.broadcast_to(cols[None] < N, vis.shape) if mutant == "sum-over-masked" else vis
                tm = best(ref, (np.where(in_max, a, ref0).min(-1) if neg else np.where(in_max, a, ref0).max(-1)))
                on = -(tm.astype(F32) * c)
                ex = _exp2(_fma(a.astype(F32), c, on[..., None]))
                s = _seq_sum(np.where(in_sum, ex, F32(0)))
                scale = {"no-rescale": np.ones_like(on), "rescale-sign": _exp2(o - on)}.get(mutant)
                l = _fma(l, _exp2(on - o) if scale is None else scale, s)
                ref, o = tm, on
            r = ref.min(1) if neg else ref.max(1)
            orow = -(r.astype(F32) * c)
            w = l if mutant == "merge-ignores-ref" else (l * _exp2(orow[:, None] - o)).astype(F32)
            total = _seq_sum(np.where(l > 0, w, F32(0)))
            inv = np.where(total > 0, F32(127) / np.where(total > 0, total, F32(1)), F32(0)).astype(F32)
            o2 = o[..., None] if mutant == "pass2-own-o" else orow[:, None, None]
            for cols, a, vis in tiles:
                ex = np.where(vis, _exp2(_fma(a.astype(F32), c, o2)), F32(0))
                y = _fma(ex, inv[:, None, None], MAGIC)
                q = (np.ascontiguousarray(y).view(np.uint32) & 0xFF).astype(np.uint8)
                keep = cols < N
                out[rows[:, None], cols[keep][None, :]] = q[:, keep]
    return out


def emulate_batch(acc, alpha, causal, mutant=None):
    return np.stack([emulate(x, alpha, causal, mutant) for x in acc])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# which family sees which fault (asserted by tests/test_softmax_adversarial_cpu.py, printed in DESIGN.md section 4.8)
# ---------------------------------------------------------------------------------------------------------------------------------------------------
# The band-rule cases of the GPU test: ("soft", shape, nats, order) | ("slot", shape, slot) | ("big",)
BAND_CASES = ([("soft", shape, nats, order) for shape in SOFT_SHAPES for nats in SOFT_NATS for order in ORDERS]
              + [("slot", shape, slot) for shape in SOFT_SHAPES for slot in range(8)] + [("big",)])
# The by-design cases: (shape, tie, alpha or None for hard_alpha(K))
HARD_CASES = ([(shape, 0, None) for shape in HARD_SHAPES] + [(shape, g, None) for shape in TIE_SHAPES for g in TIES]
              + [(shape, 0, alpha) for shape in RANGE_SHAPES for alpha in RANGE_ALPHAS])


def case_id(case):
    return "-".join(ident(c) if isinstance(c, tuple) else "hard" if c is None else f"{c:g}" if isinstance(c, float) else str(c) for c in case)


def band_operands(case, entries):
    """-> a [entries, M, K], b [entries, N, K], alpha of a BAND_CASES entry"""
    if case[0] == "soft":
        _, shape, nats, order = case
        a, b, _ = soft_operands(shape, entries, order)
        return a, b, soft_alpha(shape[1], shape[2], nats)
    if case[0] == "slot":
        return slot_case(case[1], entries, case[2])
    return big_operands(entries) + (BIG_ALPHA,)


def family_of(case):
    """the row of the fault table a case belongs to"""
    if case[0] == "soft":
        return "place" if case[3].startswith("max") else f"soft-{case[2]:g}"
    if case[0] == "slot":
        return "place"
    if case[0] == "big":
        return "big"
    shape, tie, alpha = case
    return "range" if alpha is not None else "hard-tie" if tie else "hard"


FAMILIES = ("random", "hard", "hard-tie", "soft-0.45", "soft-3", "place", "range", "big")
# family -> the mutants it rejects, full and causal taken together ("random": softmax_q8_ref's causal 130 x 70 x 200 and 300 x 257 x 130, what the suite had).
# Asserted as it stands: a family that stops seeing a fault, or starts to, is a change to look at.
_ALL, _BUT_THE_MASKED_MAX = frozenset(MUTANTS), frozenset(MUTANTS) - {"max-over-masked"}
EXPECTED_TABLE = {"random": _BUT_THE_MASKED_MAX,        # i.i.d. scores: a hidden key never leads by fp32's exponent range, and the error of o cancels
                  "hard": _ALL, "hard-tie": _ALL,
                  "soft-0.45": _BUT_THE_MASKED_MAX,     # 127 hidden keys of a tile lead by 57 nats at most: no underflow yet
                  "soft-3": _ALL, "place": _ALL, "range": _ALL,
                  "big": _BUT_THE_MASKED_MAX}           # every row sees a best key (120 keys and more are visible): a hidden one leads by nothing
