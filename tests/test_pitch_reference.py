"""The NumPy restatement of the YIN pitch tracker (tests/pitch_reference.py) against the definitions, against the reference's own walk and
against answers worked out by hand: what the GPU suite and the C ABI tests are held to has to be right first."""
import numpy as np
import pytest

import pitch_reference as R

F32, F64 = np.float32, np.float64


def test_d_truth_is_the_definition():
    rng = np.random.default_rng(1)
    for n in (2, 3, 4, 5, 7, 8, 11, 16):
        x = rng.uniform(-1, 1, n).astype(F32)
        h = n // 2
        want = [sum((float(x[i]) - float(x[i + tau])) ** 2 for i in range(h)) for tau in range(h)]
        got = R.d_truth(x)
        assert got.dtype == F64 and got.shape == (h,)
        assert np.allclose(got, want, rtol=1e-14, atol=0)
    assert R.d_truth(np.zeros(1, F32)).size == 0


def test_an_exactly_periodic_row_has_a_zero_at_its_period():
    rng = np.random.default_rng(2)
    for period, n in ((5, 40), (7, 64), (16, 101)):
        x = np.tile(rng.uniform(-1, 1, period).astype(F32), n // period + 1)[:n]
        d = R.d_truth(x)
        for multiple in range(period, n // 2, period):
            assert d[multiple] == 0.0
        assert np.all(d[1:period] > 0)
        # and d' there is exactly 0, which is what makes clean tones fragile: lowest.y * 2 is not above it
        assert R.dprime(d)[period] == 0.0


def test_the_standin_follows_the_truth_to_fp32_accuracy():
    rng = np.random.default_rng(3)
    for n in (64, 101, 256, 2048):
        x = (0.3 * np.sin(np.arange(n) * 0.07) + 0.02 * rng.normal(size=n)).astype(F32)
        t, s = R.d_truth(x), R.d_standin(x)
        assert s.dtype == F32 and s.shape == t.shape
        assert np.abs(s - t).max() <= 1e-4 * t.max()                       # measured 1e-6 ... 1.3e-5 of max d
        assert np.abs(s - t).max() > 0                                     # and it is not the truth


def test_dprime():
    d = np.array([5.0, 0.0, 0.0, 2.0, 6.0], F64)
    # d'[0] = 1; the sum is 0 at tau 1, 2: 1; tau 3: 2 * 3 / 2; tau 4: 6 * 4 / 8
    assert R.same_bits(R.dprime(d), np.array([1, 1, 1, 3, 3], F32))
    assert R.same_bits(R.dprime(np.zeros(9)), np.ones(9, F32))
    assert R.dprime(np.zeros(0)).size == 0 and R.same_bits(R.dprime(np.array([7.0])), np.ones(1, F32))
    # d is rounded to fp32 before anything else, the quotient is taken in double, the product is rounded once
    d = np.array([0.0, 1.0 + 2.0 ** -30, 3.0])
    assert R.dprime(d)[1] == F32(1.0) and R.dprime(d)[2] == F32(F64(3.0) * (2.0 / 4.0))


@pytest.mark.parametrize("name", sorted(R.PICK_ROWS))
def test_pick_on_crafted_rows(name):
    row, cutoff, minimum, want = R.PICK_ROWS[name]
    got = R.pick(row, cutoff, minimum)
    assert isinstance(got, F32)
    if want is not None:
        assert got == F32(want), (name, got)
    if np.all(np.isfinite(row)):
        assert R.same_bits(got, R.pick_literal(row, cutoff, minimum))      # the reference's loops
        literal = R.valleys_literal(row)
        X, Y = R.valleys(row)
        assert R.same_bits(X, [p[0] for p in literal]) and R.same_bits(Y, [p[1] for p in literal])


def test_pick_branches_of_the_crafted_rows():
    branch = {name: R.pick_branch(*R.PICK_ROWS[name][:3])[1] for name in R.PICK_ROWS}
    assert branch["no_valley"] == "none" and branch["x_equals_minimum"] == "none" and branch["all_ones"] == "none"
    assert branch["x_above_minimum"] == "lowest" and branch["earlier_too_high"] == "lowest"
    assert branch["lowest_nonpositive"] == "nothing" and branch["lowest_negative"] == "nothing"
    assert branch["earlier_within_factor"] == "earlier"
    assert branch["cutoff_fails"] == "lowest+cutoff" and branch["cutoff_passes"] == "lowest"
    assert branch["nan"] == "nonfinite" and branch["inf"] == "nonfinite"


def test_the_interpolated_valley_by_hand():
    row, cutoff, minimum, _ = R.PICK_ROWS["interpolated"]
    # -d' at 2, 3, 4: -.7, -.2, -.4; delta = .5 ( -.7 + .4 ) / ( -.7 + .4 - .4 ) = .5 * -.3 / -.7
    delta = F32(0.5) * (F32(-0.7) - F32(-0.4)) / (F32(-0.7) - F32(2) * F32(-0.2) + F32(-0.4))
    assert R.pick(row, cutoff, minimum) == F32(3) + delta
    X, Y = R.valleys(row)
    assert X.size == 1 and Y[0] == -(F32(-0.2) - F32(0.25) * (F32(-0.7) - F32(-0.4)) * delta)
    assert abs(float(X[0]) - (3 + 0.15 / 0.7)) < 1e-6 and Y[0] < row[3]


def test_valleys_against_the_walk_on_random_rows_with_plateaus():
    rng = np.random.default_rng(4)
    for trial in range(300):
        h = int(rng.integers(3, 80))
        levels = int(rng.integers(2, 6))                                   # few levels: plateaus, flat edges, equal depths
        row = (rng.integers(0, levels, h) / F32(levels)).astype(F32) if trial % 2 else rng.uniform(0, 2, h).astype(F32)
        literal = R.valleys_literal(row)
        X, Y = R.valleys(row)
        assert R.same_bits(X, [p[0] for p in literal]) and R.same_bits(Y, [p[1] for p in literal]), trial
        assert np.all(np.diff(X) > 0)                                      # ordered by x is ordered by index
        for minimum in (0, 3, 10):
            assert R.same_bits(R.pick(row, 0.6, minimum), R.pick_literal(row, 0.6, minimum)), trial


def test_continuity_on_crafted_vectors():
    V = R.CONTINUITY_VECTORS
    run = lambda name: R.continuity(V[name], R.CONTINUITY_SR, R.CONTINUITY_HOP)      # noqa: E731
    assert int((F32(0.1) * F32(R.CONTINUITY_SR)) / F32(R.CONTINUITY_HOP)) == R.CONTINUITY_MIN_HOPS
    assert R.same_bits(run("short_doubling"), np.full(45, 100, F32))
    assert R.same_bits(run("long_doubling_stops_the_pass"), V["long_doubling_stops_the_pass"])       # a new note, and the pass ends
    assert R.same_bits(run("doubling_of_the_note_length"), np.full(57, 100, F32))
    assert R.same_bits(run("zeros_inside_a_run"), R._vector((100, 12), (0, 3), (100, 12)))
    assert R.same_bits(run("zeros_before_a_doubling"), V["zeros_before_a_doubling"])                 # 0 -> 200 is no doubling
    assert R.same_bits(run("doubling_at_the_end"), np.full(11, 100, F32))
    assert R.same_bits(run("two_doublings"), R._vector((100, 24), (100.5, 3), (100, 10)))
    # 100 -> 200 and 200 -> 400 are both suspicious.  The first is halved over its 4 hops; the second's ratios are then taken
    # against 400 itself (still unhalved), it is 4 hops long and halved to 200
    assert R.same_bits(run("doubling_of_a_doubling"), R._vector((100, 14), (200, 4), (100, 10)))
    assert R.same_bits(run("single"), V["single"]) and R.same_bits(run("all_zero"), V["all_zero"])
    assert R.continuity(np.zeros(0, F32), 48000.0, 128).size == 0
    # a shorter note length: at hop 2048 minimum_num_hops is 2, so three hops are a new note
    assert R.same_bits(R.continuity(R._vector((100, 3), (200, 3), (100, 3)), 48000.0, 2048), R._vector((100, 3), (200, 3), (100, 3)))
    assert R.same_bits(R.continuity(R._vector((100, 3), (200, 2), (100, 3)), 48000.0, 2048), np.full(8, 100, F32))


def test_average():
    assert R.average([100, 0, 102, 0]) == F32(101)
    assert R.average([100, 0, 102, -1]) == F32(67)                          # a -1 is counted out of the valid ones and yet averaged in
    assert R.average([]) == F32(-1)                                         # 0 <= 0 * 0
    assert R.average([0, 0, 0]) == F32(0)                                   # all "valid", none non-zero: mean_and_sd of nothing
    assert R.average([-1, -1, 100], 0.5) == F32(-1) and R.average([-1, 100, 100], 0.5) == F32((F32(-1) + F32(100) + F32(100)) / F32(3))
    assert R.average([100, 104], 0.0, 1.9) == F32(-1) and R.average([100, 104], 0.0, 2.0) == F32(102)
    w = np.random.default_rng(5).uniform(50, 400, 1000).astype(F32)
    total = F32(0)
    for v in w:
        total = F32(total + v)
    assert R.average(w) == total / F32(1000)


def test_count():
    assert R.count(16000) == 109 and R.count(3000, 0, -1, 256, 32) == 86 and R.count(40, 0, -1, 6, 1) == 34
    assert R.count(2048) == 0 and R.count(2049) == 1 and R.count(2048 + 128) == 1 and R.count(2049 + 128) == 2
    assert R.count(3000, 77, 2501, 256, 32) == len(range(77, 2501 - 256, 32))
    assert R.count(100, 50, 40, 6, 1) == 0
