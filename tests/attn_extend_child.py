"""The device runs of tests/attn_extend_ref.py's identities, interval rule and staircases, as functions (tests/test_hip_attn_extend.py calls them at the default 8
waves) and as a script:

    ASQ_DECODE_WAVES=4 python tests/attn_extend_child.py 4

The library reads ASQ_DECODE_WAVES once per process, so the 4-wave and 16-wave kernels need a process of their own: the parent test starts this script once per value.
It runs identity (I2) on cases 3 and 5 (chunked, R = 16 and R = 15; the single-token entry runs with the same waves) under both signs and the two staircases.  The first
failing message goes to stdout and the exit code is 1.  As in tests/attn_decode_child.py, what the script proves is that the override was in the environment before the
library was loaded; which kernel a launch then ran is csrc/asq_attn_decode.hip's dec_waves() / launch_decode(), read, not observed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_decode_ref as R  # noqa: E402
import attn_extend_ref as X  # noqa: E402
from bmm_ref import assert_bits_equal, ref_out  # noqa: E402

DEV = "cuda:0"
CHILD_CASES = (2, 4)


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _i32(x):
    return None if x is None else torch.tensor(list(x), dtype=torch.int32, device=DEV)


def run(q, k, v, lengths, q_len, qk_alpha, pv_alpha, max_len):
    """ops.attn_extend_i8 on k, v [B, rows, Hkv, D] device buffers passed as their [:, :max_len] views; lengths / q_len: lists, tensors or None -> numpy"""
    from autosmoothquant_amd import ops
    n = lengths if torch.is_tensor(lengths) else _i32(lengths)
    m = q_len if torch.is_tensor(q_len) else _i32(q_len)
    out = ops.attn_extend_i8(q, k[:, :max_len], v[:, :max_len], n, qk_alpha, pv_alpha, q_len=m)
    assert out.dtype == torch.int8 and out.shape == q.shape and out.is_contiguous()
    return out.cpu().numpy()


def run_decode(q, k, v, lengths, qk_alpha, pv_alpha, max_len):
    from autosmoothquant_amd import ops
    return ops.attn_decode_i8(q, k[:, :max_len], v[:, :max_len], _i32(lengths), qk_alpha, pv_alpha).cpu().numpy()


def folded(qn, k, v, L, r, qk_alpha, pv_alpha, ml):
    """(I2)'s right-hand side: per token s the single-token entry on fold()'s operand -- R "heads" per KV head holding the tile rows of s's token group -- with
    kv_len' = L[:, s]; the rows of token s -> [B, Sq, Hq, D]"""
    B, sq, hq, d = qn.shape
    out = np.zeros_like(qn)
    groups = {}
    for s in range(sq):
        tg, rows = X.unfold_rows(r, sq, s)
        if tg not in groups:
            groups[tg] = dev(X.fold(qn, r, tg))[0]
        out[:, s] = run_decode(groups[tg], k, v, L[:, s].tolist(), qk_alpha, pv_alpha, ml)[:, rows(hq)]
    return out


def identity_i2(case, si, sign, with_i3=False):
    hkv, r, sq, d, lengths, q_len = X.CASES[case]
    qn, kn, vn = X.operands(case)
    q, k, v = dev(qn, kn, vn)
    L, ml, alpha = X.case_keys(case), X.max_len(lengths), sign * X.qk_alpha(case, si)
    for pv in X.PV_ALPHAS:
        what = f"{X.param_id((case, si, sign))} pv_alpha {pv:.5f}"
        got = run(q, k, v, lengths, q_len, alpha, pv, ml)
        assert_bits_equal(got, folded(qn, k, v, L, r, alpha, pv, ml), f"(I2) {what}: the extend launch against the single-token entry on the same tile rows")
        assert not got[L == 0].any(), f"{what}: a token without keys is not all zeros"
        if with_i3:
            assert not X.chunked(case)
            for s in range(sq):
                one = run_decode(q[:, s].contiguous(), k, v, L[:, s].tolist(), alpha, pv, ml)
                assert_bits_equal(got[:, s], one, f"(I3) {what}: token {s} against attn_decode_i8(q[:, {s}], kv_len = L)")


def interval_case(case, si, sign):
    hkv, r, sq, d, lengths, q_len = X.CASES[case]
    qn, kn, vn = X.operands(case)
    q, k, v = dev(qn, kn, vn)
    s_lo, s_hi, nband, total = X.case_sums(case, si, sign)
    L = X.case_keys(case)
    for pv in X.PV_ALPHAS:
        what = f"{X.param_id((case, si, sign))} pv_alpha {pv:.5f} ({'chunked ' + str(X.chunk(case)) if X.chunked(case) else 'one pass'})"
        lo, hi = R.interval(s_lo, s_hi, pv)
        amb = R.caps(lo, hi, nband, total, what)
        out = run(q, k, v, lengths, q_len, sign * X.qk_alpha(case, si), pv, X.max_len(lengths))
        print(f"{what}: {nband} of {total} P elements in the band, {amb} of {lo.size} outputs with lo != hi, {int((out != lo).sum())} outputs != lo")
        R.check(out, lo, hi, what)
        assert not out[L == 0].any(), f"{what}: a token without keys is not all zeros"


def uniform_staircase(i):
    qn, kn, vn, lengths, q_len, ml, L, s = X.uniform_staircase(i)
    q, k, v = dev(qn, kn, vn)
    for alpha in (0.01, -0.01):
        for pv in X.EXACT_PVS + (1.0,):
            assert_bits_equal(run(q, k, v, lengths, q_len, alpha, pv, ml), ref_out(s, torch.int8, pv),
                              f"uniform staircase {X.UNIFORM[i]}, qk_alpha {alpha}, pv_alpha {pv}: token s = rne(127 / L) * the sum of its first L = {L.tolist()} V rows")


def poisoned_staircase(i):
    qn, kn, vn, lengths, q_len, ml, L = X.poisoned_staircase(i)
    q, k, v = dev(qn, kn, vn)
    for pv in X.EXACT_PVS:
        assert_bits_equal(run(q, k, v, lengths, q_len, X.STAIR_ALPHA, pv, ml), X.staircase_expected(vn, L, X.STAIRS[i][1], pv),
                          f"poisoned staircase {X.STAIRS[i]}, pv_alpha {pv}: every token one-hot on its own last key, L - 1 with L = {L.tolist()}")


def main(argv):
    nw = int(argv[1])
    assert nw in (4, 16), nw
    assert os.environ.get("ASQ_DECODE_WAVES") == str(nw), f"ASQ_DECODE_WAVES is {os.environ.get('ASQ_DECODE_WAVES')!r}, not {nw}"
    assert not any(m.startswith("autosmoothquant_amd") for m in sys.modules), "the package was imported before the override was checked"
    try:
        for case in CHILD_CASES:
            for sign in X.SIGNS:
                identity_i2(case, 1, sign)
        for i in range(len(X.UNIFORM)):
            uniform_staircase(i)
        for i in range(len(X.STAIRS)):
            poisoned_staircase(i)
    except AssertionError as e:
        print(f"FAILED at {nw} waves: {e}")
        return 1
    print(f"{nw} waves: all passed")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
