"""Float64 attention as the yardstick of the int8 attention family, shared by tests/test_attn_float_cpu.py and tests/test_hip_attn_float.py.

Everything else that checks RopeQuantQKV, the int8 KV caches and Int8Attention compares integers with integers.  Here a case starts from 16-bit floating-point
q / k / v and a script of steps, and three things are computed from the same inputs:

  reference(name)         float64 softmax(q . k^T) . v in Hugging Face's formulation, per sequence over that sequence's own tokens, in output-int8 units.  It is
                          written from the definition and shares no code with tests/*_ref.py nor with model() below (it has its own RoPE, its own bookkeeping: a
                          list of live tokens per sequence).
  model(name, defect)     float64 arithmetic of the int8 pipeline AS DOCUMENTED (layers/nn/attention.py, ops.py): quantise, P = rne(127 softmax), out = sat(rne(.)),
                          with explicit caches, lengths, a block table and rewind.  defect=None is the faithful pipeline; every name in DEFECTS breaks one convention.
  the kernels' outputs    (GPU test) the public modules driven by run-script rules restated in the GPU test.

metrics() compares either of the last two with the first.  The kernels are accepted against the MODEL'S error on the same inputs (RMS_FACTOR, MAX_SLACK), never
against their own; the CPU test shows that every defect moves the error to at least CATCH_FACTOR times the faithful model's on a named case, so the acceptance
factor sits between "what the documented arithmetic costs" and "what any listed misreading costs".

A script is a list of steps (S, take, rewind): S tokens per sequence are handed to the append (right-padded), sequence b keeps take[b] of them -- token s < take[b]
sits at position length[b] + s and attends the keys up to and including its own -- and rewind[b] tokens are dropped afterwards.  A prefill is a first step, a decode
step has S = 1, a speculative step S = 4 with a per-sequence q_len.

Inputs.  q ~ N(0, 0.5), k ~ N(0, 1), v ~ N(0, 3) rounded to the case's 16-bit type; sm_scale = sd / (0.5 sqrt(D)) gives q . k^T the case's score deviation.
out_scale is the reference's absmax / 127.  q / k / v scales start from the operands' absmax / 127 (taken on the rotated values) and are only ever RAISED, by
_separate(), until the four scales differ pairwise by at least 2x: a swapped or inverted scale then changes the answer.  A raised scale costs grid levels, not
correctness, and the model pays the same price.  The envelope cases keep the plain absmax scales: they are about P's fixed step, not about a swapped scale, and
no defect is judged on them.

Planting (the float counterpart of attn_decode_ref.poisoned): in a planted case every kept token's own key is aligned with its own query (0.625 times the sum of
its group's rotated query rows, un-rotated again: a score about 2.5 deviations up) and carries a V row of +-9; and for the last kept token of every step and
sequence, the row just behind the sequence's length gets such a key as well, wherever a token wrote that row (a pad token, or one a rewind dropped since).  A key
limit off by one either way, or a rewind that is not honoured, then moves the answer at any length; without it the effect is averaged away from 64 keys on.

There is no "all rotary rows shifted by the same amount" defect: RoPE scores depend on position differences only, so such a shift changes neither the float answer
nor the int8 one beyond rounding (test_attn_float_cpu.test_a_uniform_rotary_shift_is_invisible shows it on the model).  The shift that matters is the relative
one, rope_step_off_by_one."""
import functools
import itertools
from collections import namedtuple

import numpy as np
import torch

RMS_FACTOR = 1.5       # kernels: relative RMS error <= 1.5 x the faithful model's
MAX_SLACK = 2          # kernels: max abs error <= the model's + 2
CATCH_FACTOR = 3.0     # every defect: >= 3 x the faithful model's relative RMS error on a named case
FLOOR_FACTOR = 0.67    # flat envelope cases: the kernels are at least this degraded (two-sided)
Q_WIDTH, K_WIDTH, V_WIDTH = 0.5, 1.0, 3.0
PLANT_GAIN, PLANT_V = 0.625, 9.0
PAGE = 16

Step = namedtuple("Step", "S take rewind")
Case = namedtuple("Case", "name kind hq hkv d dtype sd seed plant causal steps scored")

DEFECTS = ("kv_head_mod",            # query head h reads KV head h % Hkv instead of h // r
           "drop_own_key",           # a token sees the keys n < t, not n <= t
           "key_limit_plus_one",     # one key beyond the visible ones is attended
           "no_causal_mask",         # every token of a multi-token step sees all keys of its sequence
           "top_left",               # the tokens are placed as if all Sq counted: position kv_len - Sq + s instead of kv_len - q_len + s
           "rope_step_off_by_one",   # from the second step on, q and k are rotated with the table row one past their position
           "rope_interleaved",       # pairs (2i, 2i + 1) rotated instead of (i, i + D/2)
           "no_sm_scale",            # qk_alpha = q_scale k_scale
           "pv_alpha_inverted",      # pv_alpha = out_scale / (127 v_scale)
           "kv_scales_swapped",      # from_scale with k_scale and v_scale exchanged
           "neighbour_keys",         # sequence b reads the keys of sequence b + 1
           "pages_swapped",          # the first two pages of a sequence are read in the other order
           "rewind_ignored")         # the tokens a rewind dropped still count as keys


def _script(prompts, decodes, spec=None, after=0):
    """a padded prefill, `decodes` single-token steps, then optionally one step of 4 tokens with q_len = spec[0], a rewind of spec[1] and `after` more single tokens"""
    B = len(prompts)
    steps = [Step(max(prompts), tuple(prompts), None)] + [Step(1, (1,) * B, None)] * decodes
    if spec:
        steps += [Step(4, tuple(spec[0]), tuple(spec[1]))] + [Step(1, (1,) * B, None)] * after
    return tuple(steps)


def _case(name, kind, prompts, sd, seed, hq=8, hkv=2, d=64, dtype="fp16", plant=False, causal=True, decodes=3, spec=None, after=0, scored=None):
    steps = _script(prompts, decodes, spec, after)
    return Case(name, kind, hq, hkv, d, dtype, sd, seed, plant, causal, steps, tuple(range(len(steps))) if scored is None else tuple(scored))


_SPEC3 = ((4, 2, 3), (3, 0, 2))      # q_len per sequence, then the rejected tokens taken back
_SPEC2 = ((3, 4), (1, 4))
CASES = (
    _case("dense-fp16-n17-sd1.5", "dense", [17], 1.5, 1),
    _case("dense-bf16-n64-sd4", "dense", [64], 4.0, 2, dtype="bf16"),
    _case("dense-fp16-n300-sd4-d128", "dense", [300], 4.0, 3, d=128),
    _case("dense-fp16-n5-sd1.5-planted", "dense", [5], 1.5, 4, plant=True),
    _case("dense-noncausal-fp16-n17-sd1.5", "dense", [17], 1.5, 5, causal=False, decodes=1),
    _case("ragged-fp16-n1.5.17-sd1.5-planted", "ragged", [1, 5, 17], 1.5, 6, plant=True, decodes=2, spec=_SPEC3, after=1),
    _case("ragged-bf16-n64.17.300-sd4-planted", "ragged", [64, 17, 300], 4.0, 7, dtype="bf16", plant=True, decodes=2, spec=_SPEC3, after=1),
    _case("ragged-fp16-n5.17-sd4-mha", "ragged", [5, 17], 4.0, 8, hq=4, hkv=4, decodes=2, spec=_SPEC2, after=1),
    _case("ragged-bf16-n17.64.5-sd1.5-r8", "ragged", [17, 64, 5], 1.5, 9, dtype="bf16", hq=8, hkv=1, decodes=2, spec=_SPEC3, after=1),
    _case("paged-fp16-n17.40.5-sd1.5-planted", "paged", [17, 40, 5], 1.5, 10, plant=True, decodes=2, spec=_SPEC3, after=1),
    _case("paged-bf16-n300.64.17-sd4-planted", "paged", [300, 64, 17], 4.0, 11, dtype="bf16", plant=True, decodes=2, spec=_SPEC3, after=1),
    _case("paged-fp16-n64.1-sd4-d128", "paged", [64, 1], 4.0, 12, d=128, decodes=2, spec=_SPEC2, after=1),
    # the envelope: one decode step of one sequence over n keys (the n - 1 cached ones and its own); only that step is scored.  The issue names the last three;
    # 300 keys at a deviation of 1.5 is the row of its table where the error first leaves the few-percent range
    _case("envelope-fp16-n300-sd1.5", "envelope", [299], 1.5, 16, decodes=1, scored=[1]),
    _case("envelope-fp16-n1024-sd1", "envelope", [1023], 1.0, 13, decodes=1, scored=[1]),
    _case("envelope-fp16-n4096-sd1", "envelope", [4095], 1.0, 14, decodes=1, scored=[1]),
    _case("envelope-fp16-n4096-sd4", "envelope", [4095], 4.0, 15, decodes=1, scored=[1]),
)
BY_NAME = {c.name: c for c in CASES}
SCRIPTED = tuple(c for c in CASES if c.kind != "envelope")
ENVELOPE = tuple(c for c in CASES if c.kind == "envelope")
FLAT = ("envelope-fp16-n1024-sd1", "envelope-fp16-n4096-sd1")
_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}


def torch_dtype(case):
    return _DT[case.dtype]


def rows_needed(case):
    """the rows a sequence's cache must hold: every append writes all S rows of the step, pads included -> a multiple of the page size"""
    B = len(case.steps[0].take)
    n, need = [0] * B, 0
    for st in case.steps:
        need = max(need, max(n) + st.S)
        n = [a + t - (st.rewind[b] if st.rewind else 0) for b, (a, t) in enumerate(zip(n, st.take))]
    return -(-need // PAGE) * PAGE


def _f64(t):
    return t.double().numpy()


def _tables(T, D, dt):
    inv = 1.0 / (10000.0 ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    ang = torch.arange(T, dtype=torch.float64)[:, None] * inv[None, :]
    return ang.cos().to(dt), ang.sin().to(dt)


# ---- the reference's own RoPE: Hugging Face's apply_rotary_pos_emb ----------------------------------------------------------------------------------------------
def _rotate_half(x):
    h = x.shape[-1] // 2
    return np.concatenate([-x[..., h:], x[..., :h]], axis=-1)


def _hf_rope(x, cos, sin, pos, inverse=False):
    """x [..., H, D] float64 at table row pos; cos / sin [T, D/2] float64 -> x cos + rotate_half(x) sin with the half tables repeated (inverse: the angle negated)"""
    c, s = np.concatenate([cos[pos], cos[pos]]), np.concatenate([sin[pos], sin[pos]])
    return x * c + _rotate_half(x) * (-s if inverse else s)


class Inputs:
    """a case's operands: per step q [B, S, Hq, D], k and v [B, S, Hkv, D] as CPU tensors of the case's dtype, cos / sin [T, D/2] of that dtype, sm_scale"""

    def __init__(self, case):
        self.case = case
        dt = torch_dtype(case)
        self.B = len(case.steps[0].take)
        self.rows = rows_needed(case)
        self.cos, self.sin = _tables(self.rows + PAGE, case.d, dt)      # (room for the defects and the shift that read a later table row)
        self.sm_scale = case.sd / (Q_WIDTH * K_WIDTH * case.d ** 0.5)
        g = torch.Generator().manual_seed(57000 + case.seed)
        self.q, self.k, self.v = [], [], []
        for st in case.steps:
            self.q.append((torch.randn((self.B, st.S, case.hq, case.d), generator=g) * Q_WIDTH).to(dt))
            self.k.append((torch.randn((self.B, st.S, case.hkv, case.d), generator=g) * K_WIDTH).to(dt))
            self.v.append((torch.randn((self.B, st.S, case.hkv, case.d), generator=g) * V_WIDTH).to(dt))
        if case.plant:
            self._plant(np.random.default_rng(57500 + case.seed))

    def _plant(self, rng):
        case, cos, sin = self.case, _f64(self.cos), _f64(self.sin)
        r = case.hq // case.hkv
        writer = [dict() for _ in range(self.B)]          # row -> (step, s) of the token that wrote it last
        behind = set()
        n = [0] * self.B

        def aligned(i, b, s, pos_q, pos_k):
            """a key row at position pos_k whose rotated value is PLANT_GAIN x the group sums of token (i, b, s)'s rotated query at pos_q, and a +-PLANT_V value row"""
            q_rot = _hf_rope(_f64(self.q[i][b, s]), cos, sin, pos_q)
            k_rot = PLANT_GAIN * q_rot.reshape(case.hkv, r, case.d).sum(axis=1)
            return _hf_rope(k_rot, cos, sin, pos_k, inverse=True), PLANT_V * rng.choice([-1.0, 1.0], (case.hkv, case.d))

        def put(i, b, s, kv):
            self.k[i][b, s] = torch.from_numpy(kv[0]).to(self.k[i].dtype)
            self.v[i][b, s] = torch.from_numpy(kv[1]).to(self.v[i].dtype)

        for i, st in enumerate(case.steps):
            for b in range(self.B):
                for s in range(st.S):
                    writer[b][n[b] + s] = (i, s)
                for s in range(st.take[b]):
                    put(i, b, s, aligned(i, b, s, n[b] + s, n[b] + s))
                last = n[b] + st.take[b] - 1
                w = writer[b].get(last + 1)
                if st.take[b] and w is not None and (w[0], b, w[1]) not in behind:      # (a pad token, or one a rewind dropped: its own-key plant gives way)
                    put(w[0], b, w[1], aligned(i, b, st.take[b] - 1, last, last + 1))
                    behind.add((w[0], b, w[1]))
                n[b] += st.take[b] - (st.rewind[b] if st.rewind else 0)


@functools.lru_cache(maxsize=None)
def inputs(name):
    return Inputs(BY_NAME[name])


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------------------------
def _reference_raw(inp):
    """per step float64 [B, S, Hq, D] in v's units (None for a step that is not scored; rows of pad tokens are zero) and the mask of kept tokens [B, S]"""
    case, cos, sin = inp.case, _f64(inp.cos), _f64(inp.sin)
    r = case.hq // case.hkv
    keys, vals = [[] for _ in range(inp.B)], [[] for _ in range(inp.B)]
    outs, live = [], []
    for i, st in enumerate(case.steps):
        q, k, v = _f64(inp.q[i]), _f64(inp.k[i]), _f64(inp.v[i])
        out = np.zeros((inp.B, st.S, case.hq, case.d)) if i in case.scored else None
        for b in range(inp.B):
            first = len(keys[b])
            for s in range(st.take[b]):
                keys[b].append(_hf_rope(k[b, s], cos, sin, first + s))
                vals[b].append(v[b, s])
            if out is None or not st.take[b]:
                continue
            K = np.repeat(np.stack(keys[b]), r, axis=1)            # repeat_kv: [n, Hq, D], query head h reads KV head h // r
            V = np.repeat(np.stack(vals[b]), r, axis=1)
            Q = np.stack([_hf_rope(q[b, s], cos, sin, first + s) for s in range(st.take[b])])
            scores = np.einsum("shd,nhd->hsn", Q, K) * inp.sm_scale
            if case.causal:                                        # tril, aligned bottom-right: the last query sees every key
                n = K.shape[0]
                mask = np.tril(np.ones((st.take[b], n), dtype=bool), k=n - st.take[b])
                scores = np.where(mask[None], scores, -np.inf)
            p = np.exp(scores - scores.max(axis=-1, keepdims=True))
            p /= p.sum(axis=-1, keepdims=True)
            out[b, :st.take[b]] = np.einsum("hsn,nhd->shd", p, V)
        for b in range(inp.B):
            if st.rewind and st.rewind[b]:
                del keys[b][-st.rewind[b]:], vals[b][-st.rewind[b]:]
        outs.append(out)
        live.append(np.array([[s < t for s in range(st.S)] for t in st.take]))
    return outs, live


def _separate(tight, fixed):
    """tight: {name: absmax / 127}; fixed: out_scale.  Each scale is raised from its tight value to the smallest one at least 2x away from out_scale and from the
    scales set before it; of the six orders the one that raises least (product of the factors) is taken"""
    best = None
    for order in itertools.permutations(sorted(tight)):
        taken, got, cost = [fixed], {}, 1.0
        for name in order:
            s = tight[name]
            while any(u / 2 < s < 2 * u for u in taken):
                s = max(2 * u for u in taken if u / 2 < s < 2 * u)
            got[name] = s
            taken.append(s)
            cost *= s / tight[name]
        if best is None or cost < best[0] - 1e-12:
            best = (cost, got)
    return best[1]


Prepared = namedtuple("Prepared", "ref live q_scale k_scale v_scale out_scale raised")


@functools.lru_cache(maxsize=None)
def prepared(name):
    """the case's reference in output-int8 units, the kept-token masks and the four scales (fp32 values, as the modules hold them)"""
    inp = inputs(name)
    case, cos, sin = inp.case, _f64(inp.cos), _f64(inp.sin)
    raw, live = _reference_raw(inp)
    out_scale = float(np.float32(max(np.abs(o).max() for o in raw if o is not None) / 127))
    amax = {"q": 0.0, "k": 0.0, "v": 0.0}
    n = [0] * inp.B
    for i, st in enumerate(case.steps):         # absmax over what the quantisers see: every row handed over, pads included, q and k rotated at their positions
        for b in range(inp.B):
            for s in range(st.S):
                amax["q"] = max(amax["q"], np.abs(_hf_rope(_f64(inp.q[i][b, s]), cos, sin, n[b] + s)).max())
                amax["k"] = max(amax["k"], np.abs(_hf_rope(_f64(inp.k[i][b, s]), cos, sin, n[b] + s)).max())
            n[b] += st.take[b] - (st.rewind[b] if st.rewind else 0)
        amax["v"] = max(amax["v"], float(inp.v[i].abs().max()))
    tight = {x: float(np.float32(a / 127)) for x, a in amax.items()}          # (fp32 first: doubling one is then exact, so "at least 2x" holds exactly)
    sc = tight if case.kind == "envelope" else _separate(tight, out_scale)
    ref = [None if o is None else o / out_scale for o in raw]
    return Prepared(ref, live, sc["q"], sc["k"], sc["v"], out_scale, {x: sc[x] / tight[x] for x in sc})


def reference(name):
    """-> per step float64 [B, S, Hq, D]: softmax(sm_scale q . k^T) . v / out_scale (None for a step the case does not score)"""
    return prepared(name).ref


# ---- the model of the int8 pipeline -----------------------------------------------------------------------------------------------------------------------------
def _rope_pairs(x, cos, sin, interleaved):
    """x [H, D] rotated by one table row: pair i is (x[i], x[i + D/2]), or with `interleaved` (x[2i], x[2i + 1]); (a, b) -> (a cos - b sin, b cos + a sin)"""
    h = x.shape[-1] // 2
    out = np.empty_like(x)
    if interleaved:
        a, b = x[..., 0::2], x[..., 1::2]
        out[..., 0::2], out[..., 1::2] = a * cos - b * sin, b * cos + a * sin
    else:
        a, b = x[..., :h], x[..., h:]
        out[..., :h], out[..., h:] = a * cos - b * sin, b * cos + a * sin
    return out


def _q8(x, scale):
    return np.clip(np.rint(x / scale), -128, 127)


class _Caches:
    """int8 K / V rows of B sequences behind a block table (pages of PAGE rows handed out from a shuffled free list); a contiguous cache is the same thing with
    the identity table, so the dense, ragged and paged cases share it"""

    def __init__(self, B, rows, hkv, d, paged, seed):
        per = rows // PAGE
        self.k, self.v = np.zeros((B * per, PAGE, hkv, d)), np.zeros((B * per, PAGE, hkv, d))
        ids = np.random.default_rng(seed).permutation(B * per) if paged else np.arange(B * per)
        self.table = ids.reshape(per, B).T.copy() if paged else ids.reshape(B, per)
        self.rows = rows

    def write(self, b, row, k8, v8):
        self.k[self.table[b, row // PAGE], row % PAGE], self.v[self.table[b, row // PAGE], row % PAGE] = k8, v8

    def read(self, b, n, swap=False):
        """the first n rows of sequence b -> k, v [n, Hkv, D]; swap: table entries 0 and 1 exchanged where the n rows reach the second page"""
        pages = list(self.table[b, :-(-n // PAGE)])
        if swap and len(pages) > 1:
            pages[0], pages[1] = pages[1], pages[0]
        return self.k[pages].reshape(-1, *self.k.shape[2:])[:n], self.v[pages].reshape(-1, *self.v.shape[2:])[:n]


Modelled = namedtuple("Modelled", "out p_row_sum saturated")


def model(name, defect=None, rope_shift=0):
    """-> Modelled(per step int-valued float64 [B, S, Hq, D] (None where not scored), mean row sum of P over the scored rows, the saturated share of q8 / k8 / v8).
    rope_shift: every token rotated with the table row rope_shift past its position (not a defect: see the module docstring)"""
    assert defect is None or defect in DEFECTS
    inp, pre = inputs(name), prepared(name)
    case, cos, sin = inp.case, _f64(inp.cos), _f64(inp.sin)
    B, hq, hkv, d = inp.B, case.hq, case.hkv, case.d
    r = hq // hkv
    qs, ks, vs = pre.q_scale, pre.k_scale, pre.v_scale
    qk_alpha = qs * ks * inp.sm_scale
    pv_alpha = vs / (127 * pre.out_scale)
    if defect == "no_sm_scale":
        qk_alpha = qs * ks
    if defect == "pv_alpha_inverted":
        pv_alpha = pre.out_scale / (127 * vs)
    if defect == "kv_scales_swapped":
        qk_alpha, pv_alpha = qs * vs * inp.sm_scale, ks / (127 * pre.out_scale)
    kv_of = [(h % hkv if defect == "kv_head_mod" else h // r) for h in range(hq)]
    caches = _Caches(B, inp.rows, hkv, d, case.kind == "paged", 57900 + case.seed)
    length, ghost = [0] * B, [0] * B          # ghost: the tokens a rewind dropped, which the rewind_ignored defect still counts
    outs, row_sums, sat, total = [], [], 0, 0
    for i, st in enumerate(case.steps):
        q, k, v = _f64(inp.q[i]), _f64(inp.k[i]), _f64(inp.v[i])
        q8 = np.zeros((B, st.S, hq, d))
        for b in range(B):                  # the append: all S rows are rotated, quantised and written at length + s; the sequence then keeps take[b] of them
            for s in range(st.S):
                row = length[b] + s
                if row >= caches.rows:
                    continue
                t = row + rope_shift + (1 if defect == "rope_step_off_by_one" and i > 0 else 0)
                il = defect == "rope_interleaved"
                q8[b, s] = _q8(_rope_pairs(q[b, s], cos[t], sin[t], il), qs)
                k8, v8 = _q8(_rope_pairs(k[b, s], cos[t], sin[t], il), ks), _q8(v[b, s], vs)
                caches.write(b, row, k8, v8)
                for x in (q8[b, s], k8, v8):
                    sat += int((np.abs(x) >= 127).sum())
                    total += x.size
            length[b] += st.take[b]
        out = np.zeros((B, st.S, hq, d)) if i in case.scored else None
        for b in range(B):
            if out is None:
                break
            src = (b + 1) % B if defect == "neighbour_keys" else b
            for s in range(st.take[b]):
                pos = length[b] - (st.S if defect == "top_left" else st.take[b]) + s
                n = pos + 1 if case.causal and defect != "no_causal_mask" else length[b]
                n += (defect == "key_limit_plus_one") - (defect == "drop_own_key") + (ghost[b] if defect == "rewind_ignored" else 0)
                n = min(n, caches.rows)
                if n <= 0:
                    continue
                swap = defect == "pages_swapped" and case.kind == "paged"
                k8, _ = caches.read(src, n, swap)
                _, v8 = caches.read(b, n, swap)
                for h in range(hq):
                    sc = qk_alpha * (k8[:, kv_of[h]] @ q8[b, s, h])
                    e = np.exp(sc - sc.max())
                    p = np.rint(127 * e / e.sum())
                    out[b, s, h] = np.clip(np.rint(pv_alpha * (p @ v8[:, kv_of[h]])), -128, 127)
                    row_sums.append(p.sum())
        for b in range(B):
            if st.rewind and st.rewind[b]:
                length[b] -= st.rewind[b]
                ghost[b] += st.rewind[b]
        outs.append(out)
    return Modelled(outs, float(np.mean(row_sums)), sat / max(total, 1))


# ---- metrics ----------------------------------------------------------------------------------------------------------------------------------------------------
Metrics = namedtuple("Metrics", "rel_rms max_abs")


def metrics(name, outs):
    """outs: per step [B, S, Hq, D] (entries of unscored steps are ignored) against reference(name) over the kept tokens -> (relative RMS error, max abs error)"""
    pre = prepared(name)
    err2 = ref2 = worst = 0.0
    for o, ref, live in zip(outs, pre.ref, pre.live):
        if ref is None:
            continue
        diff = (np.asarray(o, dtype=np.float64) - ref)[live]
        err2 += float((diff ** 2).sum())
        ref2 += float((ref[live] ** 2).sum())
        worst = max(worst, float(np.abs(diff).max()))
    return Metrics((err2 / ref2) ** 0.5, worst)


@functools.lru_cache(maxsize=None)
def faithful(name):
    """-> (Metrics of model(name), its mean P row sum, its saturated share), computed once and shared"""
    m = model(name)
    return metrics(name, m.out), m.p_row_sum, m.saturated
