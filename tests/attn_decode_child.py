"""The device runs of tests/attn_decode_ref.py's exact families and of its interval rule, as functions (tests/test_hip_attn_decode.py calls them at the default 8
waves) and as a script:

    ASQ_DECODE_WAVES=4 python tests/attn_decode_child.py 4

The library reads ASQ_DECODE_WAVES once per process, so the 4-wave and 16-wave kernels need a process of their own: the parent test starts this script once per value.
It runs the key-position walk built for its own number of waves, the two weights under both signs, and the interval rule on the (1, 8, 128), (1, 16, 256) and
(1, 4, 192) cases (at 16 waves the two D > 128 cases take the documented fallback to 8).  The first failing message goes to stdout and the exit code is 1.

No entry reports which decode kernel a launch ran.  What this script proves is that the override was in the environment before the package, and so the library, was
loaded; that the library then launched the kernel the variable names is csrc/asq_attn_decode.hip's dec_waves() / launch_decode(), read, not observed."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import attn_decode_ref as R  # noqa: E402
from bmm_ref import assert_bits_equal  # noqa: E402

DEV = "cuda:0"
EXACT_PVS = (1.0 / 127, 0.003)
CHILD_CASES = [(1, 8, 128, [2047, 2049, 4100]), (1, 16, 256, [1023, 1025, 2100]), (1, 4, 192, [1, 63, 64, 65, 700])]


def dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def run(q, k, v, lengths, qk_alpha, pv_alpha, max_len, kv_len="lengths"):
    """k, v: [B, rows, Hkv, D] device buffers, passed as their [:, :max_len] views (the pitch is rows >= max_len rows)"""
    from autosmoothquant_amd import ops
    if isinstance(kv_len, str):
        kv_len = torch.tensor(lengths, dtype=torch.int32, device=DEV)
    out = ops.attn_decode_i8(q, k[:, :max_len], v[:, :max_len], kv_len, qk_alpha, pv_alpha)
    assert out.dtype == torch.int8 and out.shape == q.shape and out.is_contiguous()
    return out.cpu().numpy()


def interval_case(case, si, sign=1):
    qn, kn, vn, lengths = R.operands(case)
    q, k, v = dev(qn, kn, vn)
    s_lo, s_hi, nband, total = R.case_sums(case, si, sign)
    for pv in R.PV_ALPHAS:
        what = f"{R.param_id((case, si))}{' -qk_alpha' if sign < 0 else ''} pv_alpha {pv:.5f} ({R.form(case)})"
        lo, hi = R.interval(s_lo, s_hi, pv)
        amb = R.caps(lo, hi, nband, total, what)
        out = run(q, k, v, lengths, sign * R.qk_alpha(case, si), pv, R.max_len(lengths))
        print(f"{what}: {nband} of {total} P elements in the band, {amb} of {lo.size} outputs with lo != hi, {int((out != lo).sum())} outputs != lo")
        R.check(out, lo, hi, what)
        for b, n in enumerate(lengths):
            if n == 0:
                assert not out[b].any(), f"{what}: a sequence without keys is not all zeros"


def one_hot(made, what):
    qn, kn, vn, lengths, alpha, ml, hot = made
    q, k, v = dev(qn, kn, vn)
    for pv in EXACT_PVS:
        assert_bits_equal(run(q, k, v, lengths, alpha, pv, ml), R.one_hot_expected(vn, hot, pv), f"{what}, pv_alpha {pv}")


def walk(i, nw):
    hkv, r, d, tail = R.WALK[i]
    n, C, pos = R.walk_positions(r, nw, tail)
    print(f"walk {R.WALK[i][:3]} for {nw} waves: {n} keys in chunks of {C}, hot keys at {pos}")
    one_hot(R.walk_case(i, nw), f"key-position walk {R.WALK[i][:3]} for {nw} waves (sequence b: the hot key at {pos}[b])")


def two_weights(i, neg):
    qn, kn, vn, lengths, alpha, ml, places = R.two_weight_case(i, neg)
    q, k, v = dev(qn, kn, vn)
    r = qn.shape[1] // kn.shape[2]
    print(f"two weights {R.WALK[i][:3]}, qk_alpha {alpha:+.4f}: {lengths[0]} keys in chunks of {R.chunk(r, ml)}, (A, B) at {places}")
    for pv in EXACT_PVS:
        assert_bits_equal(run(q, k, v, lengths, alpha, pv, ml), R.two_weight_expected(vn, places, r, pv),
                          f"two weights {R.WALK[i][:3]}, qk_alpha {alpha:+.4f}, pv_alpha {pv} (sequence b: A, B at {places}[b]; 34 v[A] + 93 v[B])")


def main(argv):
    nw = int(argv[1])
    assert nw in (4, 16), nw
    assert os.environ.get("ASQ_DECODE_WAVES") == str(nw), f"ASQ_DECODE_WAVES is {os.environ.get('ASQ_DECODE_WAVES')!r}, not {nw}"
    assert not any(m.startswith("autosmoothquant_amd") for m in sys.modules), "the package was imported before the override was checked"
    try:
        for i in range(len(R.WALK)):
            walk(i, nw)
            for neg in (False, True):
                two_weights(i, neg)
        for shape in CHILD_CASES:
            for si in range(len(R.SDS)):
                interval_case(R.CASES.index(shape), si)
    except AssertionError as e:
        print(f"FAILED at {nw} waves: {e}")
        return 1
    print(f"{nw} waves: all passed")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
