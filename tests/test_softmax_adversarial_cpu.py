"""CPU: the adversarial cases of the fused softmax (tests/softmax_q8_adversarial.py) as far as they can be checked without a GPU.

For every case of tests/test_hip_bmm_softmax_adversarial.py, with the same seeds: the construction holds what it promises (levels, gaps in nats, one-hot targets,
accumulators beyond 2^24), the float64 target alone keeps the tie band under softmax_q8_ref.BAND_CAP, and the fp32 restatement of the kernel's online softmax is
accepted -- byte for byte on the by-design families.  Then the reason the cases exist: every arithmetic mutant of that restatement is rejected by at least one
family, which family rejects which is asserted as a table, and the mutant that ignores the causal mask in the running maximum passes the random causal cases the
suite had before."""
import numpy as np
import pytest

import softmax_q8_adversarial as A
import softmax_q8_ref as R

ENTRIES = max(A.BATCHES)


def hard_alpha_of(case):
    shape, _, alpha = case
    return A.hard_alpha(shape[2]) if alpha is None else alpha


def band_shares(t, N):
    """the band share of the whole batch and of its first entry (the batch-1 case of the GPU test)"""
    band = R.in_band(t, N)
    return band.mean(), band[:1].mean()


# ---- the builders ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", sorted({(s[1], s[2]) for s in A.HARD_SHAPES + A.SOFT_SHAPES}))
def test_ramp_keys_hold_their_levels(N, K):
    levels = A.ramp_levels(N, K)
    assert np.all(np.diff(levels) > 0) and levels[-1] == 127 * K and levels[0] >= -128 * K
    b = A.ramp_keys(N, K, 1)
    assert b.dtype == np.int8 and b.shape == (N, K) and np.array_equal(b.astype(np.int64).sum(1), levels)
    assert not np.array_equal(b, A.ramp_keys(N, K, 2)) and np.array_equal(b, A.ramp_keys(N, K, 1))      # seeded: other bytes, the same sums
    if K >= 64:
        assert np.all((b != b[:, :1]).any(1) | (levels % K == 0))                                        # spread over the positions, not a constant row
    for sign in (1, -1):
        acc = R.acc_exact(A.queries(np.full(3, sign), K)[None], b[None])[0]
        assert np.array_equal(acc, sign * 127 * np.broadcast_to(levels, (3, N)))                         # monotone in n for every row
    for g in A.TIES:
        tied = A.ramp_levels(N, K, g)
        assert np.all(tied[-g:] == 127 * K) and tied[-g - 1] < tied[-1] and np.all(np.diff(tied) >= 0)


def test_orders_place_the_maximum():
    for N in (257, 300):
        for name in A.ORDERS:
            src = A.order_of(name, N, 9)
            assert np.array_equal(np.sort(src), np.arange(N)), name                                      # one multiset of scores in every order
        top = lambda name: int(np.argmax(A.order_of(name, N, 9)))
        assert (top("asc"), top("desc"), top("max0"), top("max127"), top("max128"), top("maxlast")) == (N - 1, 0, 0, 127, 128, N - 1)
        assert N - 1 >= 2 * A.TILE and N % A.TILE != 0                                                   # N - 1 lies in a partial last tile
        up, down = A.order_of("saw-up", N, 9), A.order_of("saw-down", N, 9)
        for t in range(-(-N // A.TILE)):
            seg = slice(t * A.TILE, min((t + 1) * A.TILE, N))
            assert np.all(np.diff(up[seg]) == 1) and np.all(np.diff(down[seg]) == -1)
        assert up[0] > up[A.TILE] > up[2 * A.TILE] and down[0] < down[A.TILE] < down[2 * A.TILE]
    cols = [A.slot_columns(300, s) for s in range(8)]
    assert np.array_equal(np.sort(np.concatenate(cols)), np.arange(300))
    assert cols[0][:5].tolist() == [0, 1, 2, 3, 16] and cols[5][:5].tolist() == [68, 69, 70, 71, 84] and 128 in cols[0]


def test_a_causal_cut_leaves_slots_without_a_key():
    """the descending causal 300 x 300 case: row 0 sees column 0 only, so seven of its eight partials never meet a visible key (l = 0 in the merge), and the rows
    at the second tile's start repeat that with a first tile behind them"""
    none = A.slots_without_a_key(300, 300)
    assert none[0, 0].tolist() == [False] + [True] * 7 and none[128, 1].tolist() == [False] + [True] * 7
    assert none[63, 0].tolist() == [False] * 4 + [True] * 4 and not none[127, 0].any()
    assert ("soft", (300, 300, 128), 0.45, "desc") in A.BAND_CASES


# ---- by design: the hard staircase, its ties, the score range ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.HARD_CASES, ids=A.case_id)
def test_staircase_is_one_hot_for_the_mathematics_and_for_the_restatement(case):
    shape, tie, _ = case
    M, N, K = shape
    alpha = hard_alpha_of(case)
    a, b, levels, signs = A.hard_operands(shape, ENTRIES, tie)
    assert A.min_gap_nats(levels, alpha) >= A.NATS_HARD
    acc = R.acc_exact(a, b)
    assert np.array_equal(acc, 127 * signs[:, :, None] * levels[:, None, :])
    assert (signs[0] == 1).all() and (signs[1] == -1).all() and (M == 1 or len(set(signs[2])) == 2)
    if A.family_of(case) == "range":
        assert abs(alpha) * np.abs(acc).max() <= 1.04e9 and (abs(alpha) < 1e3 or abs(alpha) * np.abs(acc).max() > 2.5e8)
    for causal in (False, True):
        want, half = A.hard_want(shape, levels, signs, causal, alpha < 0)
        t = R.target(acc, alpha, causal)
        ok, _, _ = R.judge(want, t, N)
        assert ok.all()                                                                                  # the by-design bytes are what softmax_q8_ref asks for ...
        assert np.array_equal(np.rint(t)[~half], want[~half])                                            # ... with no band involved outside the two-leader rows
        assert not R.in_band(t, N)[~half].any()
        assert tie or not half.any()
        rows = R.visible(M, N, causal).any(1)
        assert np.all((want.astype(np.int64).sum(-1) > 0) == rows[None])                                # rows without a visible key are all zero
        if not tie:
            assert np.all(want.max(-1)[:, rows] == 127) and np.all((want > 0).sum(-1)[:, rows] == 1)
            if causal and alpha > 0:
                m = np.flatnonzero(rows)
                assert np.array_equal(want[0].argmax(-1)[m], m + N - M)                                 # +127 queries: 127 at n = m + N - M
                assert np.all(want[1].argmax(-1)[m] == 0)                                               # -127 queries: at 0
        elif not causal:
            assert np.all(want[0][:, -tie:] == round(127 / tie)) and not want[0][:, :-tie].any()          # the g best keys share the row
        A.check_one_hot(A.emulate_batch(acc, alpha, causal), want, half, f"restatement {A.case_id(case)} causal={causal}")


@pytest.mark.parametrize("path", list(A.FORM_SHAPES))
@pytest.mark.parametrize("form", list(A.FORMS))
def test_head_operands_of_the_kernel_forms(form, path):
    """the operands of the grouped and token-major calls: each key head its own staircase, the query heads of a group differ in sign; the staircase is exact for the
    restatement and the soft ramp stays under the band cap"""
    S, h, r = A.FORMS[form]
    shape = M, N, K = A.FORM_SHAPES[path]
    for ties in (True, False):
        a, b, levels, signs = A.head_operands(shape, S, h, r, ties)
        assert a.shape == (S * h, M, K) and b.shape == (S * h // r, N, K)
        assert len({x.tobytes() for x in b}) == len(b) and (r == 1 or len({s.tobytes() for s in signs[:r]}) >= 2)
        acc = R.acc_exact(a, b[np.arange(S * h) // r])
        alpha = A.hard_alpha(K) if ties else A.soft_alpha(N, K, 0.45)
        for causal in (False, True):
            if ties:
                assert min(A.min_gap_nats(lv, alpha) for lv in levels) >= A.NATS_HARD
                want, half = A.head_want(shape, levels, signs, r, causal)
                assert R.judge(want, R.target(acc, alpha, causal), N)[0].all()
                A.check_one_hot(A.emulate_batch(acc, alpha, causal), want, half, f"{form} {path} causal={causal}")
            else:
                R.check(A.emulate_batch(acc, alpha, causal), R.target(acc, alpha, causal), N, f"{form} {path} causal={causal}")


def test_the_staircase_check_sees_one_byte():
    shape = (16, 300, 128)
    a, b, levels, signs = A.hard_operands(shape, 1, 0)
    want, half = A.hard_want(shape, levels, signs, True)
    A.check_one_hot(want, want, half)
    for (m, n, v) in ((0, 0, 1), (15, 299, 126), (7, 291, 0), (7, 292, 127)):
        q = want.copy()
        q[0, m, n] = v
        with pytest.raises(AssertionError, match="differ from the staircase"):
            A.check_one_hot(q, want, half)
    tied = A.hard_operands(shape, 1, 4)
    want, half = A.hard_want(shape, tied[2], tied[3], True)
    assert half.any() and set(np.unique(want)) == {0, 32, 42, 64, 127}
    q = want.copy()
    q[want == 64] = 63
    A.check_one_hot(q, want, half)                                                                       # 63.5 may round either way ...
    q[want == 42] = 43
    with pytest.raises(AssertionError):
        A.check_one_hot(q, want, half)                                                                   # ... nothing else may


# ---- band rule: the soft ramps, the placed maxima, the slots, accumulators beyond 2^24 ---------------------------------------------------------------
@pytest.mark.parametrize("case", A.BAND_CASES, ids=A.case_id)
def test_band_cases_stay_under_the_cap_and_accept_the_restatement(case):
    a, b, alpha = A.band_operands(case, ENTRIES)
    N = b.shape[1]
    acc = R.acc_exact(a, b)
    for causal in (False, True):
        t = R.target(acc, alpha, causal)
        for share in band_shares(t, N):
            assert share <= R.BAND_CAP, (A.case_id(case), causal, share)
        R.check(A.emulate_batch(acc, alpha, causal), t, N, f"restatement {A.case_id(case)} causal={causal}")


def test_soft_ramp_gaps_in_nats():
    for shape in A.SOFT_SHAPES:
        M, N, K = shape
        levels = A.ramp_levels(N, K)
        for nats in A.SOFT_NATS:
            alpha = A.soft_alpha(N, K, nats)
            gap = A.min_gap_nats(levels, alpha)
            assert abs(gap - nats) < 1e-3 * nats and np.all(np.diff(levels) == levels[1] - levels[0])
        # at 3 nats per key the hidden keys of a diagonal-cut tile lead the row's own best key by more than NATS_FAR within the tile's 128 columns
        assert 3.0 * (A.TILE - 1) > 2 * A.NATS_FAR
        for slot in range(8):
            a, b, alpha = A.slot_case(shape, 1, slot)
            lv = b[0].astype(np.int64).sum(1)
            cols = A.slot_columns(N, slot)
            rest = np.setdiff1d(np.arange(N), cols)
            assert 127 * alpha * (lv[cols].min() - lv[rest].max()) >= A.NATS_FAR and lv[cols].max() == 127 * K
            assert abs(A.min_gap_nats(lv[cols], alpha) - 0.45) < 1e-3


def test_big_accumulators():
    a, b = A.big_operands(ENTRIES)
    acc = R.acc_exact(a, b)
    assert acc.max() > 2 ** 24 and acc.max() == 2 ** 25 and not (acc % 4096).any()
    assert np.array_equal(acc.astype(np.float32).astype(np.int64), acc)                                  # exact in fp32
    below = np.unique(acc.max() - acc) * np.float64(np.float32(A.BIG_ALPHA))
    assert below[0] == 0 and 1.5 <= below[1] < 1.6 and below[2] > 100 and len(below) == 3
    top = acc[:, 0] == acc.max()
    assert np.all(top.sum(-1) == 3) and np.all(top[:, A.TILE:].sum(-1) >= 1)                             # a best key behind the tile seam, hidden from the first rows
    assert not np.array_equal(b[0], b[1])


def test_alphas_of_no_effect_give_uniform_targets():
    a, b = R.operands((40, 24, 64), 2)
    acc = R.acc_exact(a, b)
    for alpha in A.NULL_ALPHAS:
        for causal in (False, True):
            t = R.target(acc, alpha, causal)
            assert np.abs(t - R.target(np.zeros_like(acc), 0.37, causal)).max() < 1e-9
            assert np.array_equal(A.emulate_batch(acc, alpha, causal), A.emulate_batch(np.zeros_like(acc), 0.37, causal))
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny


def test_the_score_domain_of_the_restatement_ends_at_2_31():
    """why the range cases stop at |alpha acc| = 1e9: o = fl(-float(ref) * c) carries half an ulp of ref * c, 64 below |c acc| = 2^31 and 128 or 256 beyond it, which exp2
    no longer holds -- at K = 272 and alpha = 1e3 (|c acc| up to 2.96 * 2^31) the restatement loses every full row.  DESIGN.md section 4.8 states the domain."""
    shape = (257, 129, 272)
    a, b, levels, signs = A.hard_operands(shape, 1, 0)
    acc = R.acc_exact(a, b)
    assert np.abs(acc).max() * 1e3 * 1.4427 > 2.9 * 2.0 ** 31
    assert not A.emulate_batch(acc, 1e3, False).any()
    for shape in A.RANGE_SHAPES:
        assert 127 * 127 * shape[2] * max(A.RANGE_ALPHAS) * 1.4427 < 2.0 ** 31


# ---- the faults --------------------------------------------------------------------------------------------------------------------------------------
def rejects(family, mutant):
    """does any case of the family, full or causal, reject the mutated restatement?  (The unmutated one passes all of them: the tests above.)"""
    if family == "random":
        for shape in ((130, 70, 200), (300, 257, 130)):
            a, b = R.operands(shape, 1)
            acc = R.acc_exact(a, b)
            for alpha in R.alphas(shape):
                if not R.judge(A.emulate_batch(acc, alpha, True, mutant), R.target(acc, alpha, True), shape[1])[0].all():
                    return True
        return False
    for case in A.HARD_CASES:
        if A.family_of(case) != family:
            continue
        shape, tie, _ = case
        a, b, levels, signs = A.hard_operands(shape, ENTRIES, tie)
        acc = R.acc_exact(a, b)
        for causal in (True, False):
            want, half = A.hard_want(shape, levels, signs, causal, hard_alpha_of(case) < 0)
            try:
                A.check_one_hot(A.emulate_batch(acc, hard_alpha_of(case), causal, mutant), want, half)
            except AssertionError:
                return True
    for case in A.BAND_CASES:
        if A.family_of(case) != family:
            continue
        a, b, alpha = A.band_operands(case, ENTRIES)
        acc = R.acc_exact(a, b)
        for causal in (True, False):
            if not R.judge(A.emulate_batch(acc, alpha, causal, mutant), R.target(acc, alpha, causal), b.shape[1])[0].all():
                return True
    return False


@pytest.mark.parametrize("mutant", A.MUTANTS)
@pytest.mark.parametrize("family", A.FAMILIES)
def test_fault_table(family, mutant):
    got = rejects(family, mutant)
    print(f"TABLE {family} {mutant} {got}")
    assert got == (mutant in A.EXPECTED_TABLE[family]), f"{family} {'rejects' if got else 'accepts'} {mutant}"


def test_every_mutant_is_rejected_somewhere_and_the_old_cases_miss_the_mask():
    assert set(A.EXPECTED_TABLE) == set(A.FAMILIES)
    new = set().union(*(A.EXPECTED_TABLE[f] for f in A.FAMILIES if f != "random"))
    assert new == set(A.MUTANTS)
    assert "max-over-masked" not in A.EXPECTED_TABLE["random"]                                           # the gap the adversarial cases close
    for family in ("hard", "hard-tie", "soft-3"):
        assert "max-over-masked" in A.EXPECTED_TABLE[family]


def test_the_masked_maximum_fault_in_rows():
    """the mutant that takes the running maximum over the hidden columns of a diagonal-cut tile: accepted on every element of the random causal cases, rejected in
    every +127 row of the causal staircase that sees a key and whose block walks a column the row does not see"""
    for shape in ((130, 70, 200), (300, 257, 130)):
        a, b = R.operands(shape, 1)
        acc = R.acc_exact(a, b)
        for alpha in R.alphas(shape):
            ok, _, _ = R.judge(A.emulate_batch(acc, alpha, True, "max-over-masked"), R.target(acc, alpha, True), shape[1])
            assert ok.all(), (shape, alpha)
    for shape, rows in (((300, 300, 128), 297), ((130, 257, 33), 129)):
        M, N, K = shape
        a, b, levels, signs = A.hard_operands(shape, 1, 0)
        want, _ = A.hard_want(shape, levels, signs, True)
        q = A.emulate_batch(R.acc_exact(a, b), A.hard_alpha(K), True, "max-over-masked")
        bad = (q != want).any(-1)[0]
        last = np.arange(M) + N - M                                                                      # the row's own column ...
        block_last = np.minimum(np.arange(M) // A.TILE * A.TILE + A.TILE, M) - 1 + N - M                 # ... and that of its block's last row
        end = np.minimum((block_last + A.TILE) // A.TILE * A.TILE, N)                                    # the columns the block walks
        assert bad.sum() == rows and np.array_equal(bad, (last >= 0) & (last < end - 1))                 # a hidden key among them: the row is lost
        assert not q[0][bad].any()                                                                       # such rows come out all zero
