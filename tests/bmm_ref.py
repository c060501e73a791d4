"""What the GPU tests of the batched int8 matmuls share (test_hip_bmm.py, test_hip_bmm_kn.py, test_hip_bmm_softmax.py): the epilogues restated in
numpy, the bit-pattern views, the mismatch report and the in-run timer.  The exact accumulators stay with each file: they are independent yardsticks."""
import numpy as np
import torch


def ref_out(acc, kind, alpha):
    if kind == torch.int32:
        return acc
    y = np.float32(alpha) * acc.astype(np.float32)   # one fp32 product, int -> float rounded to nearest even
    if kind == torch.float32:
        return y.astype(np.float32)
    return np.clip(np.rint(y), -128, 127).astype(np.int8)


def bits(x):
    """bit patterns (f32 outputs compared as integers: -0.0 != 0.0, NaN == NaN)"""
    x = np.ascontiguousarray(x)
    return x.view(np.int32) if x.dtype == np.float32 else x


def tbits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_bits_equal(got, want, what):
    """got, want: numpy arrays of one shape and dtype; `what` names the case in the report"""
    if not np.array_equal(bits(got), bits(want)):
        bad = np.argwhere(bits(got) != bits(want))
        raise AssertionError(f"{what}: {len(bad)} mismatches, first at {bad[0]}: got {got[tuple(bad[0])]} want {want[tuple(bad[0])]}")


def medians_us(fns, nrot, reps=20, warm=5):
    """per function the median HIP-event time of one call, the functions alternating call by call (the same clocks and neighbours for all of them)"""
    for i in range(warm):
        for fn in fns:
            fn(i % nrot)
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for i in range(reps):
        for j, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn((i + warm) % nrot)
            e.record()
            e.synchronize()
            times[j].append(s.elapsed_time(e) * 1e3)
    return [float(np.median(t)) for t in times]
