"""No GPU: what tests/test_hip_fp8_exact.py stands on (tests/fp8_exact.py).
  - the builders' premises on every case of the GPU table: the codes decode to the intended values, sum |x w| / q < 2^24 for every output, the sparse case's
    |acc| < 2^8, the MX scale variety;
  - with power-of-two scales and biases that are multiples of 2^-4 the restated epilogue equals oracle.fp8.easy_fp8_gemm (e5m2: the same expression on
    e5m2_to_f32 values) and oracle.mx.mx_linear bit for bit in f32, f16 and bf16: the new yardstick is tied to the reference-pinned oracle;
  - restated faults: the exact comparison on the new operands rejects every one; today's tolerance rule on today's operands rejects the gross ones (the table is
    printed, and copied into DESIGN.md);
  - the dispatcher sends every shape of the GPU table to the class the table names, by default and under every forced ASQ_GEMM_KERNEL."""
import numpy as np
import pytest

import detrng
import fp8_exact as X
from oracle import fp8 as F8
from oracle import mx as MX
from oracle import w8a8 as O

F32 = np.float32


def test_grids_are_what_the_formats_hold():
    assert np.array_equal(X.grid_values("e4m3"), np.arange(-15.0, 16.0))
    pos = [0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16]
    assert sorted(X.grid_values("e5m2")) == sorted(set(pos) | {-v for v in pos})
    for fmt in ("e4m3", "e5m2"):   # every grid value times every row spread is a code of the format
        v = (X.grid_values(fmt)[None, :] * X.row_spread(3)).reshape(-1)
        assert np.array_equal(X.DEC[fmt](X.ENC[fmt](v.astype(F32))).astype(np.float64), v)


@pytest.mark.parametrize("cls,shape", X.TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_premises_on_the_default_dispatch_table(cls, shape):
    for fmt in ("e4m3", "e5m2"):
        for kind in ("grid",) + (("sparse",) if shape in X.SPARSE_SHAPES else ()):
            c = X.linear_case(kind, fmt, *shape)   # (decode, bound, multiple of q and the sparse 2^8 are asserted inside)
            assert np.array_equal(X.DEC[fmt](c.xq).astype(np.float64), c.x) and np.array_equal(X.DEC[fmt](c.wq).astype(np.float64), c.w)
            assert c.bound < X.LIMIT and c.bound <= 2.0 ** 21   # far inside: K <= 1152, |x w| <= 16 x 16, q = 2^-2
            if kind == "sparse":
                assert np.abs(c.acc).max() < 2.0 ** 8 and np.array_equal(O.round_to(c.acc.astype(F32), "bf16"), c.acc.astype(F32))
                assert shape[2] < 128 or (c.acc != 0).mean() > 0.2   # (still a test: a fair share of the outputs is non-zero)
            else:
                assert len(np.unique(c.acc)) > min(c.acc.size, 64) // 2


def test_premises_on_the_other_cases():
    shapes = set(X.FORCED_SHAPES) | {s for _, s in X.NAN_SHAPES} | {X.PREMISE}
    for shape in sorted(shapes - {s for _, s in X.TABLE}):
        for fmt in ("e4m3", "e5m2"):
            assert X.linear_case("grid", fmt, *shape).bound < X.LIMIT
    for _, shape in X.SUBNORMAL_SHAPES:
        c = X.linear_case("subnormal", "e4m3", *shape)
        assert c.q == 2.0 ** -18 and np.abs(c.x).max() == 7 * 2.0 ** -9 and ((c.xq & 0x78) == 0).all() and (c.acc != 0).mean() > 0.9
    for counts in X.GROUP_COUNTS:
        for N in X.GROUP_N:
            c = X.group_case(counts, N, X.GROUP_K)
            o = 0
            for g, n in enumerate(counts):   # a group's rows against that group's weight
                assert np.array_equal(c.acc[o:o + n], c.x[o:o + n] @ c.w[g].T)
                o += n
    for _, shape in X.MX_SHAPES + [("fallback", X.MX_FALLBACK), ("premise", X.PREMISE)]:
        c = X.mx_case(*shape)
        assert c.bound < X.LIMIT and set(np.unique(c.xs)) <= {126, 127, 128} and np.abs(c.xv).max() == 7
        assert (c.xs[:, 1:] != c.xs[:, :-1]).all() and (c.M < 2 or (c.xs[1:] != c.xs[:-1]).all()) and (c.N < 2 or (c.ws[1:] != c.ws[:-1]).all())
        assert len(np.unique(c.xs)) == 3 and len(np.unique(c.ws)) == 3


@pytest.mark.parametrize("dt", X.DTS)
def test_restated_epilogue_equals_the_oracle_at_power_of_two_scales(dt):
    for kind, fmt, shape in [("grid", "e4m3", (17, 65, 384)), ("grid", "e5m2", (17, 65, 384)), ("sparse", "e4m3", (17, 65, 384)), ("sparse", "e5m2", (17, 65, 384)),
                             ("grid", "e4m3", (5, 130, 129)), ("grid", "e5m2", (1, 1, 1)), ("subnormal", "e4m3", (17, 65, 256))]:
        c = X.linear_case(kind, fmt, *shape)
        s_row, s_t, s_w, bias = X.epilogue_operands(c.M, c.N, True, tag=c.K)
        assert np.array_equal(bias * 16, np.rint(bias * 16)) and (np.log2(s_row) % 1 == 0).all()
        for a_scale, sr in ((s_row.reshape(-1, 1), s_row), (s_t, s_t)):
            for b in (None, bias):
                X.same(X.epilogue_restated(c.acc, sr, s_w, b, dt), X.oracle_gemm(fmt, c.xq, a_scale, c.wq, s_w, b, dt), "%s %s %s" % (kind, fmt, dt))
    # grouped: per-group power-of-two weight scales and bias[g]
    for counts in X.GROUP_COUNTS:
        c = X.group_case(counts, X.GROUP_N[1], X.GROUP_K)
        s_row = X.epilogue_operands(c.M, c.N, True)[0]
        sg, gb = X.group_operands(c.G, c.N)
        assert len(np.unique(sg)) == c.G
        got = X.epilogue_restated(c.acc, s_row, sg[c.grp], gb[c.grp], dt)
        o = 0
        for g, n in enumerate(counts):
            if n:
                X.same(got[o:o + n], F8.easy_fp8_gemm(c.xq[o:o + n], s_row[o:o + n].reshape(-1, 1), c.wq[g], sg[g], gb[g], dt), "group %d %s" % (g, dt))
            o += n
    # MX: unit epilogue scales, the block scales inside the product
    for shape in ((33, 100, 192), (129, 129, 512)):
        c = X.mx_case(*shape)
        for b in (None, X.mx_bias(c.N)):
            X.same(X.epilogue_restated(c.acc, F32(1), F32(1), b, dt), MX.mx_linear(c.xq, c.xs, c.wq, c.ws, b, dt), "mx %s" % dt)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# restated faults: today's rule on today's operands, the exact comparison on the new ones
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def _close(got, ref, rtol):   # tests/test_hip_fp8.py::close
    return np.abs(got - ref).max() <= rtol * np.abs(ref).max() + 1e-30


def _todays_cases(dt):
    """the operands of test_fp8_linear_vs_oracle at 130 x 264 x 384 (per-token, bias), of test_fp8_grouped_launch_vs_per_group_oracle and of
    test_mx_linear_vs_oracle at 130 x 264 x 384, with each test's own acceptance rule: rule(fp32 output of a kernel) -> accepted?"""
    M, N, K = 130, 264, 384
    x = O.round_to(detrng.act_like(202, M, (M, K), scale=3.0), dt)
    W = (detrng.normal(203, N, (N, K)) * F32(0.02)).astype(F32)
    b = (detrng.normal(204, N, (N,)) * F32(0.5)).astype(F32)
    wq, ws = F8.per_tensor_quantize_fp8(W, "f32")
    aq, a_s = F8.per_token_quantize_fp8(x, dt)
    ref = O.round_to(F8.easy_fp8_gemm(aq, a_s, wq, ws, b, "f32"), dt)
    tol = {"f32": 1e-3, "f16": 2e-3, "bf16": 1e-2}[dt]
    dec = lambda q: F8.e4m3fn_to_f32(q).astype(np.float64)
    linear = (X.fault_case(dec(aq), dec(wq), a_s.reshape(-1), F32(ws), b), lambda out: _close(O.round_to(out, dt), ref, tol))
    cases = {"linear": linear, "subnormal": linear}
    # grouped (fp16 activations, fp32 output, 1e-3 per group)
    if dt == "f32":
        counts = [300, 0, 17, 256, 1, 130]
        G, Ng, Kg, Mg = len(counts), 320, 256, sum(counts)
        xg = O.round_to(detrng.act_like(210, Mg, (Mg, Kg), scale=3.0), "f16")
        gq, g_s = F8.per_token_quantize_fp8(xg, "f16")
        gw = [F8.per_tensor_quantize_fp8((detrng.normal(211, g, (Ng, Kg)) * F32(0.02 * (g + 1))).astype(F32), "f32") for g in range(G)]
        gb = (detrng.normal(212, G, (G, Ng)) * F32(0.5)).astype(F32)
        grp = np.repeat(np.arange(G), counts)
        bounds = np.concatenate([[0], np.cumsum(counts)])
        refs = [F8.easy_fp8_gemm(gq[bounds[g]:bounds[g + 1]], g_s[bounds[g]:bounds[g + 1]], gw[g][0], gw[g][1], gb[g], "f32") if counts[g] else None for g in range(G)]
        acc = np.concatenate([dec(gq[bounds[g]:bounds[g + 1]]) @ dec(gw[g][0]).T for g in range(G)])
        rule = lambda out: all(_close(out[bounds[g]:bounds[g + 1]], refs[g], 1e-3) for g in range(G) if counts[g])
        cases["grouped"] = (X.fault_case(None, None, g_s.reshape(-1), np.array([gw[g][1] for g in grp], F32), gb[grp], acc=acc), rule)
    # MX
    xm = O.round_to(detrng.act_like(710, M, (M, K), scale=2.0), dt)
    wm = (detrng.normal(711, N, (N, K)) * 0.05).astype(F32)
    bm = detrng.normal(712, N, (N,)).astype(F32)
    (xq, xs), (mq, ms) = MX.mx_quantize_e4m3(xm), MX.mx_quantize_e4m3(wm)
    mref = MX.mx_linear(xq, xs, mq, ms, bm, dt)
    mtol = (1e-3 if dt != "bf16" else 8e-3) * max(1.0, float(np.abs(mref).max()))
    cases["mx"] = (X.fault_case(MX.mx_dequantize(xq, xs), MX.mx_dequantize(mq, ms), F32(1), F32(1), bm, xv=dec(xq), xs=xs),
                   lambda out: np.abs(O.round_to(out, dt) - mref).max() <= mtol)
    return cases


def _new_cases():
    """the new operands each fault is judged on, with the restatement as the reference"""
    c = X.linear_case("grid", "e4m3", 17, 65, 384)
    s_row, _, s_w, bias = X.epilogue_operands(c.M, c.N, False, tag=c.K)
    s = X.linear_case("subnormal", "e4m3", 17, 65, 256)
    p_row, _, p_w, p_bias = X.epilogue_operands(s.M, s.N, True, tag=s.K)
    g = X.group_case(X.GROUP_COUNTS[0], X.GROUP_N[0], X.GROUP_K)
    sg, gb = X.group_operands(g.G, g.N)
    m = X.mx_case(33, 100, 192)
    return {"linear": X.fault_case(c.x, c.w, s_row, s_w, bias, acc=c.acc), "subnormal": X.fault_case(s.x, s.w, p_row, p_w, p_bias, acc=s.acc),
            "grouped": X.fault_case(None, None, X.epilogue_operands(g.M, g.N, True)[0], sg[g.grp], gb[g.grp], acc=g.acc),
            "mx": X.fault_case(m.x, m.w, F32(1), F32(1), X.mx_bias(m.N), xv=m.xv, xs=m.xs, acc=m.acc)}


GROSS = ("last 16 k of one row dropped", "row M-1 finished with row M-2's scale")   # ISSUE: these move an output by 0.66 and 1.5 against a budget of <= 0.142


def test_restated_faults():
    new = _new_cases()
    todays = {dt: _todays_cases(dt) for dt in X.DTS}
    for dt in X.DTS:   # the rules accept the unfaulted restatement of their own operands (the table below is about the faults alone)
        for name, (case, rule) in todays[dt].items():
            assert rule(X.finish(case)), (dt, name)
    rows = []
    for name, fault, on in X.FAULTS:
        missed = {dt: (todays[dt][on][1](fault(todays[dt][on][0])) if on in todays[dt] else None) for dt in X.DTS}
        bad = X.differs(fault(new[on]), X.finish(new[on]))
        rows.append((name, missed, int(bad.sum())))
    word = {True: "passes", False: "rejected", None: "-"}
    print("\n| fault | today's rule f32 | f16 | bf16 | exact comparison: elements that differ |\n| --- | --- | --- | --- | --- |")
    for name, missed, nbad in rows:
        print("| %s | %s | %s | %s | %d |" % (name, word[missed["f32"]], word[missed["f16"]], word[missed["bf16"]], nbad))
    for name, missed, nbad in rows:
        assert nbad > 0, "the exact comparison misses: " + name
        if name in GROSS:
            assert not any(missed.values()), "today's rule misses a gross fault: " + name


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the dispatcher reaches the class each table names
# ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_every_class_sees_every_scale_variant():
    for cls in {c for c, _ in X.TABLE}:
        seen = set()
        for c, shape in X.TABLE:
            if c == cls:
                seen |= set(X.variants_of(X.class_index(c, shape), shape))
        assert seen == set(X.VARIANTS), cls


def test_dispatcher_reaches_the_intended_classes():
    from autosmoothquant_amd import _lib as L
    table = X.TABLE + X.SUBNORMAL_SHAPES[1:] + X.NAN_SHAPES + [("generic", X.PREMISE)]
    got = X.names_in_child(L.LIB_PATH, None, [s for _, s in table])
    assert got == [c for c, _ in table], [(c, s, g) for (c, s), g in zip(table, got) if c != g]
    for env in X.FORCED:
        shapes = X.FORCED_SHAPES + ([X.SUBNORMAL_SHAPES[0][1]] if env == "generic" else [])
        assert X.names_in_child(L.LIB_PATH, env, shapes) == [env] * len(shapes), env
    assert X.names_in_child(L.LIB_PATH, None, X.FORCED_SHAPES + [X.SUBNORMAL_SHAPES[0][1]]) == ["p8h", "skinny", "skinny"]   # (not what the forced children run)
