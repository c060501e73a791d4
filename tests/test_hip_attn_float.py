"""GPU: RopeQuantQKV, the int8 KV caches and Int8Attention, through the public modules only, against float64 attention (tests/attn_float_ref.py).

Every case starts from 16-bit floating-point q / k / v and a script of steps; each step's int8 output is compared with reference() for that step:

  dense      RopeQuantQKV + Int8KVCache + Int8Attention(layout="bshd"), B = 1: a prefill and decode steps; the same int8 operands permuted through the head-major
             forward as well (the b_group route for a causal prefill, the fold route for a decode step and for the non-causal prefill);
  ragged     RaggedInt8KVCache: a padded prefill of unequal lengths (extend with q_len = the prompts), decode steps, one four-token extend with a per-sequence q_len,
             rewind of the rejected tokens, another decode step;
  paged      the same script on PagedInt8KVCache with pages of 16 rows, cache.free shuffled first: no sequence's pages are ascending or adjacent;
  envelope   one decode step of one sequence over 300 / 1024 / 4096 keys.

Acceptance per case, against the float64 MODEL of the documented pipeline on the same inputs, never against the kernels' own error: relative RMS error <= 1.5 x the
model's, max abs error <= the model's + 2.  The CPU test shows that every listed misreading of a convention costs at least 3 x.  The two flat envelope cases are
two-sided: the kernels' error is also >= 0.67 x the model's, so the collapse of long flat rows is pinned as a property of the design.  Each test prints the kernels'
error, the model's and their ratio (DESIGN.md 4.16 keeps the measured ratios)."""
import random

import numpy as np
import pytest
import torch

import attn_float_ref as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _modules(name):
    from autosmoothquant_amd.layers.nn.attention import Int8Attention, RopeQuantQKV
    inp, pre = F.inputs(name), F.prepared(name)
    mod = RopeQuantQKV(pre.q_scale, pre.k_scale, pre.v_scale).to(DEV)
    att = Int8Attention.from_scale(pre.q_scale, pre.k_scale, pre.v_scale, pre.out_scale, sm_scale=inp.sm_scale, causal=inp.case.causal).to(DEV)
    return inp, mod, att, inp.cos.to(DEV), inp.sin.to(DEV)


def _host(t):
    return t.cpu().numpy().astype(np.float64)


def _vec(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=DEV)


def run_dense(name):
    """-> {"bshd": per-step outputs, "bhsd": the same int8 operands through the head-major forward}"""
    from autosmoothquant_amd.layers.nn.attention import Int8KVCache
    inp, mod, att, cos, sin = _modules(name)
    case = inp.case
    cache = Int8KVCache(1, inp.rows, case.hkv, case.d, device=DEV)
    outs = {"bshd": [], "bhsd": []}
    for i, st in enumerate(case.steps):
        assert st.take == (st.S,) and not st.rewind
        q8, k8, v8 = mod(inp.q[i].to(DEV), inp.k[i].to(DEV), inp.v[i].to(DEV), cos, sin, cache=cache)
        outs["bshd"].append(_host(att(q8, k8, v8, layout="bshd")))
        hm = att(*(x.permute(0, 2, 1, 3).contiguous() for x in (q8, k8, v8)))
        outs["bhsd"].append(_host(hm.permute(0, 2, 1, 3)))
    torch.cuda.synchronize()
    return outs


def _scattered(pages):
    return len(pages) < 2 or (pages != sorted(pages) and all(abs(a - c) != 1 for a, c in zip(pages, pages[1:])))


def _shuffle_free(cache, first, B, seed):
    """cache.free shuffled (the first seed from `seed` on that does it) so that the `first` pages each of the B sequences takes in its first step, handed out
    from the end of the free list, are neither ascending nor adjacent; run_cached asserts it on cache.pages after that step"""
    for j in range(256):
        free = list(cache.free)
        random.Random(seed + j).shuffle(free)
        order = free[::-1]
        if all(_scattered(order[b * first:(b + 1) * first]) for b in range(B)):
            break
    cache.free[:] = free


def run_cached(name):
    """the ragged, paged and envelope scripts -> per-step outputs (None for a step the case does not score: the append alone runs)"""
    from autosmoothquant_amd.layers.nn.attention import PagedInt8KVCache, RaggedInt8KVCache
    inp, mod, att, cos, sin = _modules(name)
    case, B = inp.case, inp.B
    paged = case.kind == "paged"
    if paged:
        per = inp.rows // F.PAGE
        cache = PagedInt8KVCache(B * per + 5, F.PAGE, case.hkv, case.d, B, inp.rows, device=DEV)
        _shuffle_free(cache, -(-case.steps[0].S // F.PAGE), B, 58000 + case.seed)
    else:
        cache = RaggedInt8KVCache(B, inp.rows, case.hkv, case.d, device=DEV)
    outs = []
    for i, st in enumerate(case.steps):
        q8, kc, vc = mod(inp.q[i].to(DEV), inp.k[i].to(DEV), inp.v[i].to(DEV), cos, sin, cache=cache, advance=list(st.take))
        assert cache.lengths == cache.kv_len.tolist()
        if i not in case.scored:
            outs.append(None)
        elif st.S == 1:
            out = att.decode_paged(q8, kc, vc, cache.block_table, cache.kv_len, max_len=cache.bound()) if paged else att.decode(q8, kc, vc, cache.kv_len, max_len=cache.bound())
            outs.append(_host(out))
        else:
            q_len = _vec(st.take)
            out = (att.extend_paged(q8, kc, vc, cache.block_table, cache.kv_len, q_len=q_len, max_len=cache.bound()) if paged
                   else att.extend(q8, kc, vc, cache.kv_len, q_len=q_len, max_len=cache.bound()))
            out = _host(out)
            for b, t in enumerate(st.take):
                assert not out[b, t:].any(), f"{name}, step {i}, sequence {b}: a pad token's row is not zero"
            outs.append(out)
        if paged and i == 0:
            for b, pg in enumerate(cache.pages):
                if len(pg) > 1:
                    assert _scattered(pg), f"{name}: sequence {b}'s pages {pg} are ascending or adjacent"
        if st.rewind:
            cache.rewind(list(st.rewind))
    torch.cuda.synchronize()
    return outs


def judge(name, outs, what):
    """prints kernel error, model error and their ratio; asserts the acceptance rule -> the ratio of the relative RMS errors"""
    got, (want, row_sum, _) = F.metrics(name, outs), F.faithful(name)
    ratio = got.rel_rms / want.rel_rms
    print(f"{name} [{what}]: kernels rel rms {got.rel_rms:.4f} max {got.max_abs:.2f} | model rel rms {want.rel_rms:.4f} max {want.max_abs:.2f} (P row sum {row_sum:.1f}) | "
          f"ratio {ratio:.3f}")
    assert got.rel_rms <= F.RMS_FACTOR * want.rel_rms, f"{name} [{what}]: relative RMS error {got.rel_rms:.4f} against float attention, the model's is {want.rel_rms:.4f}"
    assert got.max_abs <= want.max_abs + F.MAX_SLACK, f"{name} [{what}]: max abs error {got.max_abs:.2f} against float attention, the model's is {want.max_abs:.2f}"
    return ratio


@pytest.mark.parametrize("name", [c.name for c in F.CASES if c.kind == "dense"])
def test_dense_cache_prefill_and_decode_steps(name):
    outs = run_dense(name)
    for route in ("bshd", "bhsd"):
        judge(name, outs[route], route)


@pytest.mark.parametrize("name", [c.name for c in F.CASES if c.kind in ("ragged", "paged")])
def test_ragged_and_paged_scripts(name):
    judge(name, run_cached(name), F.BY_NAME[name].kind)


@pytest.mark.parametrize("name", [c.name for c in F.ENVELOPE])
def test_envelope_decode_step(name):
    """the same rule; the flat cases are as degraded as the model predicts, not less: P's fixed 1 / 127 step loses the row"""
    ratio = judge(name, run_cached(name), "decode")
    if name in F.FLAT:
        assert ratio >= F.FLOOR_FACTOR, f"{name}: the kernels' error is {ratio:.2f} x the model's: the documented pipeline predicts the collapse the kernels do not show"
