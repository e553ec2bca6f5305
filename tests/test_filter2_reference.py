"""The NumPy restatement of Audio::filter_2pole_* and the shelves (tests/filter2_reference.py) against itself and against what the filters
must do: the scan model meets the conditions the device is held to on every case, the section lists give the gains resonant and doubled
Butterworth filters have at their cutoff, the NaN rule of odd orders, the two classes of cases.  No device."""
import numpy as np
import pytest

import filter_reference as R1
import filter2_reference as R

F32, F64 = np.float32, np.float64
# the conditions tests/test_gpu_filter2.py puts on the device
REL_RMS_BOUND, REL_MAX_BOUND, TRUTH_FACTOR, TRUTH_FLOOR = R.REL_RMS_BOUND, R.REL_MAX_BOUND, R.TRUTH_FACTOR, R.TRUTH_FLOOR


@pytest.mark.parametrize("name", R.CHECKED_IDS)
def test_the_scan_model_meets_the_conditions(name):
    """the proof that a correct implementation can pass the case table: both classes against the truth, parity cases against the loop too"""
    c = R.case(name)
    want, truth = R.expected(name, F32), R.expected(name, F64)
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(truth))
    own_rms, own_max = R.errors(want, truth, c["x"])
    for run in (1, 7, 16, 64):
        got = R.call(c, run=run)
        assert got.dtype == F32 and got.shape == c["x"].shape
        rms, mx = R.errors(got, truth, c["x"])
        p_rms, p_max = R.errors(got, want, c["x"])
        print("%s run %d: vs truth %.3e %.3e (the fp32 loop: %.3e %.3e); vs the loop %.3e %.3e" % (name, run, rms, mx, own_rms, own_max, p_rms, p_max))
        assert rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and mx <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR), (name, run)
        if c["cls"] == R.PARITY:
            assert p_rms <= REL_RMS_BOUND and p_max <= REL_MAX_BOUND, (name, run)


def missed(name, n, figures):
    """prints every window's figures of a row of n frames at a run of 1, then returns the windows that miss the conditions
    tests/test_gpu_filter2.py puts on the device"""
    out = []
    for (_, lo, hi), (label, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max)) in zip(R.windows(n, 1), figures):
        print("%s %s: vs the fp32 loop %.3e %.3e; vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % (name, label, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
        if not (rel_rms <= R.rms_bound(lo, hi) and rel_max <= REL_MAX_BOUND):
            out.append((label, "loop", rel_rms, rel_max))
        if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
            out.append((label, "truth", t_rms, t_max, own_rms, own_max))
    return out


@pytest.mark.parametrize("name", ["low2_d025_n131857_run1", "highshelf3_dcurve_p6_n131857_run1", "highshelf3_dcurve_p6_n65537_run1"])
def test_the_scan_model_meets_the_conditions_past_one_pass_of_the_carry(name):
    """what tests/test_gpu_filter2.py asks of the device on rows of more than 256 blocks, whole and window by window, a correct scan gives"""
    c = R.long_case(name)
    got = R.call(c, run=1)
    n = c["x"].shape[1]
    assert [w[0] for w in R.windows(n, 1)] == ["whole", "pass 0", "pass 1", "pass 1 head", "pass 2", "pass 2 head"][:6 if n > 2 * R.PASS_RUNS else 4]
    assert R.windows(R.PASS_RUNS + 1, 1)[2:] == [("pass 1", R.PASS_RUNS, R.PASS_RUNS + 1), ("pass 1 head", R.PASS_RUNS, R.PASS_RUNS + 1)]
    assert R.rms_bound(0, 256) == REL_RMS_BOUND and R.rms_bound(0, 255) == R.SHORT_WINDOW_REL_RMS_BOUND > REL_RMS_BOUND       # the one-frame pass alone
    failures = missed(name, n, R.figures(got, R.long_expected(name, F32), R.long_expected(name, F64), c["x"], 1))
    assert not failures, failures


def test_a_state_lost_between_two_passes_misses_the_conditions_where_it_is_lost():
    """the carry kernel forgetting its state at the start of its second pass: frames from 65 536 on are filtered from zero states.  The
    first block of the pass misses its allowance 1e4 times over; 8192 frames on the filter has forgotten"""
    name = "low2_d025_n131857_run1"
    c = R.long_case(name)
    cut = R.PASS_RUNS
    broken = np.concatenate([R.filter2(c["x"][:, :cut], c["sr"], c["cutoff"][:cut], c["damping"], c["gain"], c["kind"], c["order"], run=1),
                             R.filter2(c["x"][:, cut:], c["sr"], c["cutoff"][cut:], c["damping"], c["gain"], c["kind"], c["order"], run=1)], axis=1)
    want, truth = R.long_expected(name, F32), R.long_expected(name, F64)
    by_label = {f[0]: f for f in R.figures(broken, want, truth, c["x"], 1)}
    assert {"whole", "pass 1", "pass 1 head"} <= {m[0] for m in missed("lost state", c["x"].shape[1], by_label.values())}
    _, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max) = by_label["pass 1 head"]
    assert rel_rms >= 1e4 * REL_RMS_BOUND and rel_max >= 1e4 * REL_MAX_BOUND
    assert t_rms >= 1e4 * max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max >= 1e4 * max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)
    later = cut + 8192
    n = c["x"].shape[1]
    rel = R.errors_over(broken, want, c["x"], later, n)
    t, own = R.errors_over(broken, truth, c["x"], later, n), R.errors_over(want, truth, c["x"], later, n)
    print("lost state, from frame %d on: vs the fp32 loop %.3e %.3e; vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % ((later,) + rel + t + own))
    assert rel[0] <= REL_RMS_BOUND and rel[1] <= REL_MAX_BOUND
    assert t[0] <= max(TRUTH_FACTOR * own[0], TRUTH_FLOOR) and t[1] <= max(TRUTH_FACTOR * own[1], TRUTH_FLOOR)


def test_what_frames_0_to_255_leave_at_the_later_passes():
    """whether new input in frames [0, 256) still moves the output at frames 65 536 and 131 072 of the damping 0.25 low-pass: it does
    not.  Under the swept cutoff (200 Hz at frame 0, rising) a pole of damping 0.25 decays by about exp( -0.25 * 2 pi 200 / 48000 ) a frame
    or faster, which is exp( -400 ) over a pass: the scan model gives the same bits at both frames.  So tests/test_gpu_filter2.py holds no
    such property on this case, and tests/test_gpu_filter.py holds it on a 1 Hz low-pass, which remembers"""
    name = "low2_d025_n131857_run1"
    c = R.long_case(name)
    x = c["x"].copy()
    x[:, :256] = R.noise(3, 256, 77) * F32(3)
    a, b = R.call(c, run=1), R.call(c, run=1, x=x)
    assert not np.array_equal(a[:, :256], b[:, :256])
    for frame in (R.PASS_RUNS, 2 * R.PASS_RUNS):
        assert np.array_equal(a[:, frame].view(np.uint32), b[:, frame].view(np.uint32)), frame
    assert np.exp(-0.25 * 2 * np.pi * 200.0 / R.SR * R.PASS_RUNS) < 1e-150


def test_a_1_hz_low_pass_of_damping_1_remembers_frames_0_to_255_two_passes_on():
    """the case tests/test_gpu_filter2.py uses instead: order 1 at damping 1 is one section with both poles at the cutoff.  The scan
    model's output moves by more than 8 ulps at frames 65 536 and 131 072 in every channel"""
    x, other = R.memory_inputs()
    a = R.filter2(x, R.SR, R.MEMORY_CUTOFF, 1.0, 0.0, R.LOW, 1, run=1)
    b = R.filter2(other, R.SR, R.MEMORY_CUTOFF, 1.0, 0.0, R.LOW, 1, run=1)
    for frame in (R.PASS_RUNS, 2 * R.PASS_RUNS):
        moved = np.abs(a[:, frame].astype(F64) - b[:, frame].astype(F64)) / np.spacing(np.abs(a[:, frame]))
        print("frame %d: moved by %s ulps" % (frame, moved))
        assert np.all(moved > 8.0), frame


def test_one_run_of_the_scan_model_is_the_sequential_loop():
    for name in ("n1_low3", "n15_highshelf4", "n16_band2"):
        got = R.call(R.case(name), run=16)
        assert np.array_equal(got.view(np.uint32), R.expected(name, F32).view(np.uint32)), name


def test_the_two_classes():
    assert len(R.TRUTH_ONLY_IDS) * 6 <= len(R.PARITY_IDS) + len(R.TRUTH_ONLY_IDS)
    assert sorted(R.TRUTH_ONLY_IDS) == sorted(R.TRUTH_ONLY_NAMES) and len(R.TRUTH_ONLY_NAMES) == 7
    resonances = [n for n in R.TRUTH_ONLY_IDS if n.endswith("res002")]
    shelves = [n for n in R.TRUTH_ONLY_IDS if n.startswith("shelf1")]
    assert len(resonances) == 3 and len(shelves) == 4 and len(resonances) + len(shelves) == len(R.TRUTH_ONLY_IDS)
    for n in resonances:
        assert R.case(n)["damping"] == 0.02
    for n in shelves:
        assert R.case(n)["kind"] in (R.SHELF1_LOW, R.SHELF1_HIGH) and R.case(n)["order"] in (2, 3)
    # membership is by name alone: every other 1-pole shelf and every damping of 0.1 and more is a parity case
    for c in R.CASES:
        if c["cls"] == R.PARITY:
            assert not (c["kind"] <= R.SHELF1_HIGH and c["order"] >= 2), c["name"]
            assert np.min(np.asarray(c["damping"])) >= 0.1 - 1e-6, c["name"]


def test_the_case_table_covers_what_it_should():
    lengths = {c["x"].shape[1] for c in R.CASES}
    assert {1, 15, 16, 17, 1023, 1025, 4095, 4097, 12305, 4096, 12304} <= lengths
    assert {c["x"].shape[0] for c in R.CASES} == {1, 2, 3}
    have = {(c["kind"], c["order"]) for c in R.CASES if c["cls"]}
    for kind in range(9):
        orders = (0, 1, 2, 3) if kind <= R.SHELF1_HIGH else (0, 1, 2, 3, 4)
        assert {(kind, o) for o in orders} <= have, kind
    assert not [c for c in R.CASES if c["kind"] <= R.SHELF1_HIGH and c["order"] > 3]
    scalar = lambda v: np.isscalar(v)                                  # noqa: E731
    forms = {(scalar(c["cutoff"]), scalar(c["damping"]), scalar(c["gain"])) for c in R.CASES if c["cls"]}
    assert (True, True, True) in forms and (False, False, False) in forms and len(forms) >= 5      # scalar, all-curve and mixed arguments
    for c in R.CASES:
        assert c["x"].shape[0] <= 3 and c["x"].shape[1] <= 12305
        if c["cls"] and c["kind"] > R.SHELF1_HIGH and np.max(np.asarray(c["damping"])) > 0.9 + 1e-6:
            assert c["order"] % 2 == 0 and np.max(np.asarray(c["damping"])) <= 1.5 + 1e-6, c["name"]      # past 1 with even orders only
    assert any(np.max(np.asarray(c["damping"])) > 1.0 and c["order"] in (2, 4) for c in R.CASES if c["cls"])
    gains = [c["gain"] for c in R.CASES if c["cls"] and (c["kind"] <= R.SHELF1_HIGH or c["kind"] >= R.LOWSHELF)]
    assert 6.0 in [g for g in gains if np.isscalar(g)] and -12.0 in [g for g in gains if np.isscalar(g)]
    assert any(not np.isscalar(g) and abs(np.max(g) - 12.0) < 0.1 and abs(np.min(g) + 12.0) < 0.1 for g in gains)
    quads = [c for c in R.CASES if c["cls"] == R.PARITY and c["x"].shape[1] % 4 == 0 and c["x"].shape[1] >= R.BLOCK]
    assert {c["x"].shape[1] for c in quads} == {4096, 12304} and {c["x"].shape[0] for c in quads} == {2, 3} and len(quads) == 8


def _amplitude_at(y, hz):
    """the amplitude of the hz component of y over its second half, by least squares"""
    n = len(y)
    t = np.arange(n) / R.SR
    half = slice(n // 2, n)
    basis = np.stack([np.cos(2 * np.pi * hz * t[half]), np.sin(2 * np.pi * hz * t[half])], axis=1)
    coef, *_ = np.linalg.lstsq(basis, np.asarray(y, F64)[half], rcond=None)
    return float(np.hypot(coef[0], coef[1]))


def _tone(hz):
    return np.sin(2 * np.pi * hz * np.arange(R.N3) / R.SR).astype(F32)[None, :]


@pytest.mark.parametrize("damping", [0.25, 0.7071])
def test_order_1_is_one_state_variable_section(damping):
    """a sine AT the cutoff: low and high come out at 1 / ( 2 R ), the band (bp * 2 R) at 1"""
    hz = 3000.0
    x = _tone(hz)
    for kind, want in ((R.LOW, 0.5 / damping), (R.HIGH, 0.5 / damping), (R.BAND, 1.0)):
        amp = _amplitude_at(R.filter2(x, R.SR, hz, damping, 0.0, kind, 1, F64)[0], hz)
        print("R %.4f kind %d: amplitude %.6f, want %.6f" % (damping, kind, amp, want))
        assert abs(amp - want) <= 1e-3


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_damping_1_doubles_every_butterworth_pole(order):
    """at R = 1 the scaler is 1: p1 = p2 = the Butterworth pole, the real pole's section has R = 1 (two 1-pole sections).  So the low-pass
    is the Butterworth low-pass of that order applied twice: exactly half at the cutoff"""
    hz = 3000.0
    x = _tone(hz)
    amp = _amplitude_at(R.filter2(x, R.SR, hz, 1.0, 0.0, R.LOW, order, F64)[0], hz)
    once = R1.filter_1pole(x, R.SR, hz, R1.BUTTERWORTH_LOW, order, F64)
    twice = _amplitude_at(R1.filter_1pole(once, R.SR, hz, R1.BUTTERWORTH_LOW, order, F64)[0], hz)
    print("order %d: amplitude %.8f, the order-N low-pass twice %.8f" % (order, amp, twice))
    assert abs(amp - 0.5) <= 1e-3 and abs(amp - twice) <= 1e-5
    assert [p for p, _, _, _ in R.sections(R.LOW, order)] == [2] * order          # order N is N state-variable sections
    roles = [role for _, _, role, _ in R.sections(R.LOW, order)]
    assert roles == ([R.REAL_POLE] if order % 2 else []) + [R.POLE_TIMES, R.POLE_OVER] * (order // 2)


def test_the_tilt_sections():
    assert [(p, o, r) for p, o, r, _ in R.sections(R.SHELF1_LOW, 3)] == [(1, R.MIX_TILT1, R.TILT_1POLE), (2, R.MIX_TILT2, R.TILT_2POLE)]
    assert [(p, o, r) for p, o, r, _ in R.sections(R.SHELF1_HIGH, 4)] == [(2, R.MIX_TILT2, R.TILT_2POLE)] * 2
    assert R.sections(R.NOTCH, 0) == [] and R.sections(R.SHELF1_LOW, 0) == []
    # the 2-pole sections' R = Re( pole ) / w is negative and tiny (:479)
    _, Rrow, _ = R.section_rows(R.SHELF1_LOW, 2, R.TILT_2POLE, R.poles(2)[0], 1000.0, 0.0, 6.0, R.SR, 4)
    assert np.all(Rrow < 0) and np.all(Rrow > -1e-3)


def test_a_damping_above_1_makes_odd_orders_nan_from_that_frame_on():
    damping = R.damping_curve(R.N3, 0.1, 1.5)
    first = int(np.argmax(damping > 1.0))
    assert 0 < first < R.N3 and damping[first - 1] <= 1.0
    x = R.noise(1, R.N3, 31)
    for order in (1, 3):
        out = R.filter2(x, R.SR, 1000.0, damping, 0.0, R.LOW, order)
        assert not np.any(np.isnan(out[:, :first])) and np.all(np.isnan(out[:, first:])), order
        scan = R.filter2(x, R.SR, 1000.0, damping, 0.0, R.LOW, order, run=16)
        assert not np.any(np.isnan(scan[:, :first])) and np.all(np.isnan(scan[:, first:])), order
    for order in (2, 4):
        assert np.all(np.isfinite(R.filter2(x, R.SR, 1000.0, damping, 0.0, R.LOW, order))), order
    # the band shelf's damping * M passes 1 where the damping does not
    out = R.filter2(x, R.SR, 1000.0, 0.9, -12.0, R.BANDSHELF, 1)
    assert np.all(np.isnan(out))
    # one frame above 1 poisons what follows and nothing before
    got, clean = R.expected("over1_highshelf3"), R.expected("clean_highshelf3")
    f = R.POISON_FRAME
    assert np.array_equal(got[:, :f].view(np.uint32), clean[:, :f].view(np.uint32)) and np.all(np.isnan(got[:, f:]))
    got, clean = R.expected("nan_low3"), R.expected("clean_low3")
    assert np.array_equal(got[:, :f].view(np.uint32), clean[:, :f].view(np.uint32)) and np.all(np.isnan(got[:, f:]))


def test_order_zero():
    x = R.noise(2, 100, 3)
    for kind in (R.LOW, R.BAND, R.HIGH, R.LOWSHELF, R.BANDSHELF, R.HIGHSHELF):
        assert np.array_equal(R.filter2(x, R.SR, 1000.0, 0.5, 6.0, kind, 0).view(np.uint32), x.view(np.uint32)), kind
    assert not np.any(R.filter2(x, R.SR, 1000.0, 0.5, 6.0, R.NOTCH, 0))
    half = F32(np.power(10.0, F64(F32(3.0) / F32(20))))
    for kind in (R.SHELF1_LOW, R.SHELF1_HIGH):
        assert np.array_equal(R.filter2(x, R.SR, 1000.0, 0.5, 6.0, kind, 0).view(np.uint32), (x * half).view(np.uint32)), kind
