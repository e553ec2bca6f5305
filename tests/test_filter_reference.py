"""The NumPy restatement of Audio::filter_1pole_* (tests/filter_reference.py) against itself and against what a Butterworth filter must
do: the scan model meets the condition the device is held to on every case, the cutoff sits at -3 dB, low + high give the input back, the
dampings, order 0, the NaN cutoff.  No device."""
import numpy as np
import pytest

import filter_reference as R

F32, F64 = np.float32, np.float64
# the condition tests/test_gpu_filter.py puts on the device (compress's): against the fp64 truth at most 4 x the fp32 loop's own error on
# the same case, or 8 fp32 ulps of the input's scale where that is smaller
TRUTH_FACTOR = 4.0
TRUTH_FLOOR = 8 * 2.0 ** -23


@pytest.mark.parametrize("name", R.PARITY_IDS)
def test_the_scan_model_meets_the_truth_condition(name):
    """the proof that a correct implementation can pass the case table"""
    c = R.case(name)
    truth = R.expected(name, F64)
    own_rms, own_max = R.errors(R.expected(name, F32), truth, c["x"])
    for run in (1, 7, 16, 64):
        got = R.filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"], run=run)
        assert got.dtype == F32 and got.shape == c["x"].shape
        rms, mx = R.errors(got, truth, c["x"])
        print("%s run %d: vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % (name, run, rms, mx, own_rms, own_max))
        assert rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and mx <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR), (name, run)


# against the fp32 loop: the bounds of tests/test_gpu_filter.py
REL_RMS_BOUND = 1.2e-7
REL_MAX_BOUND = 6.0e-7


def missed(name, figures):
    """prints every window's figures, then returns the windows that miss the conditions tests/test_gpu_filter.py puts on the device"""
    out = []
    for label, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max) in figures:
        print("%s %s: vs the fp32 loop %.3e %.3e; vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % (name, label, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
        if not (rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND):
            out.append((label, "loop", rel_rms, rel_max))
        if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
            out.append((label, "truth", t_rms, t_max, own_rms, own_max))
    return out


@pytest.mark.parametrize("name", ["low3_n131857_run1", "high2_n131857_run1", "low3_n1052688"])
def test_the_scan_model_meets_the_conditions_past_one_pass_of_the_carry(name):
    """what tests/test_gpu_filter.py asks of the device on rows of more than 256 blocks, whole and window by window, a correct scan gives"""
    c = R.long_case(name)
    run = c["run"] or R.RUN
    got = R.filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"], run=run)
    assert [w[0] for w in R.windows(c["x"].shape[1], run)] == (["whole", "pass 0", "pass 1", "pass 1 head", "pass 2", "pass 2 head"] if c["run"] else
                                                                 ["whole", "pass 0", "pass 1", "pass 1 head"])
    failures = missed(name, R.figures(got, R.long_expected(name, F32), R.long_expected(name, F64), c["x"], run))
    assert not failures, failures


def test_a_state_lost_between_two_passes_misses_the_conditions_where_it_is_lost():
    """the carry kernel forgetting its state at the start of its second pass: frames from 65 536 on are filtered from a zero state.  The
    first block of the pass misses its allowance 1e4 times over; 8192 frames on the filter has forgotten, which is why the whole-signal
    figures are not enough and the windows are there"""
    name = "low3_n131857_run1"
    c = R.long_case(name)
    cut = R.PASS_RUNS
    broken = np.concatenate([R.filter_1pole(c["x"][:, :cut], c["sr"], c["cutoff"][:cut], c["kind"], c["order"], run=1),
                             R.filter_1pole(c["x"][:, cut:], c["sr"], c["cutoff"][cut:], c["kind"], c["order"], run=1)], axis=1)
    want, truth = R.long_expected(name, F32), R.long_expected(name, F64)
    by_label = {f[0]: f for f in R.figures(broken, want, truth, c["x"], 1)}
    _, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max) = by_label["pass 1 head"]
    print("lost state, pass 1 head: vs the fp32 loop %.3e %.3e; vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % (rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
    assert rel_rms >= 1e4 * REL_RMS_BOUND and rel_max >= 1e4 * REL_MAX_BOUND
    assert t_rms >= 1e4 * max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max >= 1e4 * max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)
    assert {"whole", "pass 1", "pass 1 head"} <= {m[0] for m in missed("lost state", by_label.values())}
    later = cut + 8192
    n = c["x"].shape[1]
    rel = R.errors_over(broken, want, c["x"], later, n)
    t, own = R.errors_over(broken, truth, c["x"], later, n), R.errors_over(want, truth, c["x"], later, n)
    print("lost state, from frame %d on: vs the fp32 loop %.3e %.3e; vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % ((later,) + rel + t + own))
    assert rel[0] <= REL_RMS_BOUND and rel[1] <= REL_MAX_BOUND
    assert t[0] <= max(TRUTH_FACTOR * own[0], TRUTH_FLOOR) and t[1] <= max(TRUTH_FACTOR * own[1], TRUTH_FLOOR)


def test_a_1_hz_low_pass_remembers_frames_0_to_255_two_passes_on():
    """the case tests/test_gpu_filter.py uses to see the state flow through a whole pass of the carry kernel: under the swept cutoffs
    nothing of frames [0, 256) is left at frame 65 536, under a 1 Hz first-order low-pass the state decays by exp( -2 pi / 48000 ) a
    frame, 1.9e-4 over a pass and 3.5e-8 over two.  The scan model's output moves by more than 8 ulps at both frames in every channel"""
    x, other = R.memory_inputs()
    a = R.filter_1pole(x, R.SR, R.MEMORY_CUTOFF, R.BUTTERWORTH_LOW, 1, run=1)
    b = R.filter_1pole(other, R.SR, R.MEMORY_CUTOFF, R.BUTTERWORTH_LOW, 1, run=1)
    assert np.array_equal(x[:, 256:], other[:, 256:])
    for frame in (R.PASS_RUNS, 2 * R.PASS_RUNS):
        moved = np.abs(a[:, frame].astype(F64) - b[:, frame].astype(F64)) / np.spacing(np.abs(a[:, frame]))
        print("frame %d: moved by %s ulps" % (frame, moved))
        assert np.all(moved > 8.0), frame


def test_one_run_of_the_scan_model_is_the_sequential_loop():
    for name in ("n1_low3_noise_sweep", "n15_high4_noise_wobble", "n16_rlow16_sine_random"):
        c = R.case(name)
        got = R.filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"], run=16)
        assert np.array_equal(got.view(np.uint32), R.expected(name, F32).view(np.uint32)), name


def test_the_case_table_covers_what_it_should():
    lengths = {c["x"].shape[1] for c in R.CASES}
    assert {1, 15, 16, 17, 1023, 1025, 4095, 4097, 12305} <= lengths
    assert {c["x"].shape[0] for c in R.CASES} == {1, 2, 3}
    have = {(c["kind"], c["order"]) for c in R.CASES}
    for kind in (R.BUTTERWORTH_LOW, R.BUTTERWORTH_HIGH):
        assert {(kind, o) for o in (0, 1, 2, 3, 4, 8)} <= have
    for kind in (R.REPEAT_LOW, R.REPEAT_HIGH):
        assert {(kind, o) for o in (0, 1, 16)} <= have
    for c in R.CASES:
        assert c["x"].shape[0] <= 3 and c["x"].shape[1] <= 12305
        if c["parity"]:
            assert np.all(np.asarray(c["cutoff"]) <= 0.45 * R.SR), c["name"]
    quads = [c for c in R.CASES if c["parity"] and c["x"].shape[1] % 4 == 0 and c["x"].shape[1] >= R.BLOCK]     # the 16-byte loads, many blocks
    assert {c["x"].shape[1] for c in quads} == {4096, 12304} and {c["x"].shape[0] for c in quads} == {2, 3}
    assert {(R.BUTTERWORTH_LOW, 2), (R.BUTTERWORTH_HIGH, 3), (R.BUTTERWORTH_LOW, 8), (R.BUTTERWORTH_HIGH, 8), (R.BUTTERWORTH_LOW, 3),
            (R.BUTTERWORTH_HIGH, 2), (R.REPEAT_LOW, 16), (R.REPEAT_HIGH, 3)} <= {(c["kind"], c["order"]) for c in quads}
    assert R.stalls("dc_20hz_low2")                        # the fp32 loop stops short of the level it approaches
    assert not R.stalls("low8_noise_sweep")


@pytest.mark.parametrize("order", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("kind", [R.BUTTERWORTH_LOW, R.BUTTERWORTH_HIGH], ids=["low", "high"])
def test_the_cutoff_sits_at_minus_3_db(kind, order):
    """a sine AT the cutoff comes out at 1 / sqrt( 2 ) whatever the order: prewarping makes that exact.  3000 Hz is 16 samples a period"""
    n, hz = 4800, 3000.0
    t = np.arange(n) / R.SR
    x = np.sin(2 * np.pi * hz * t).astype(F32)[None, :]
    y = R.filter_1pole(x, R.SR, hz, kind, order)[0].astype(F64)
    tail = slice(n - 1600, n)                              # 100 whole periods, the transient long gone
    c, s = np.cos(2 * np.pi * hz * t[tail]), np.sin(2 * np.pi * hz * t[tail])
    amp = 2.0 * np.hypot(np.dot(y[tail], c), np.dot(y[tail], s)) / 1600
    print("order %d: amplitude %.9f, off 1/sqrt(2) by %.2e" % (order, amp, abs(amp * np.sqrt(2.0) - 1.0)))
    assert abs(amp * np.sqrt(2.0) - 1.0) <= 1e-5


def test_first_order_low_plus_high_is_the_input():
    for name in ("low1_noise_sweep", "high1_sine_random"):
        c = R.case(name)
        low = R.filter_1pole(c["x"], c["sr"], c["cutoff"], R.BUTTERWORTH_LOW, 1)
        high = R.filter_1pole(c["x"], c["sr"], c["cutoff"], R.BUTTERWORTH_HIGH, 1)
        ulp = np.spacing(F32(np.max(np.abs(c["x"]))))
        assert np.max(np.abs((low.astype(F64) + high.astype(F64)) - c["x"])) <= ulp


def test_butterworth_dampings():
    assert [float(r) for r in R.butterworth_R(2)] == [float(F32(0.70710677))]
    assert [float(r) for r in R.butterworth_R(3)] == [float(F32(0.50000006))]
    assert [float(r) for r in R.butterworth_R(8)] == [float(F32(v)) for v in (0.19509032, 0.55557036, 0.83146966, 0.9807853)]
    assert R.butterworth_R(1) == [] and R.butterworth_R(0) == []
    assert [p for p, _, _ in R.sections(R.BUTTERWORTH_LOW, 5)] == [1, 2, 2]          # the 1-pole section first
    assert [p for p, _, _ in R.sections(R.BUTTERWORTH_HIGH, 4)] == [2, 2]
    assert R.sections(R.REPEAT_HIGH, 3) == [(1, F32(0), R.HIGH)] * 3


def test_order_zero_copies_and_no_repeats_are_silence():
    for name in ("low0_noise_1k", "high0_noise_wobble"):
        assert np.array_equal(R.expected(name).view(np.uint32), R.case(name)["x"].view(np.uint32)), name
    for name in ("rlow0_noise_1k", "rhigh0_sine_random"):
        assert R.expected(name).shape == R.case(name)["x"].shape and not np.any(R.expected(name)), name


def test_a_nan_cutoff_poisons_what_follows_and_nothing_before():
    got, clean = R.expected("nan_low3"), R.expected("clean_low3")
    f = R.NAN_FRAME
    assert np.isnan(R.coefficients(R.case("nan_low3")["cutoff"], R.SR, R.N3)[f])    # std::clamp by comparisons keeps it
    assert np.array_equal(got[:, :f].view(np.uint32), clean[:, :f].view(np.uint32))
    assert np.all(np.isnan(got[:, f:]))
    scan = R.filter_1pole(R.case("nan_low3")["x"], R.SR, R.case("nan_low3")["cutoff"], R.BUTTERWORTH_LOW, 3, run=16)
    assert np.all(np.isnan(scan[:, f:])) and not np.any(np.isnan(scan[:, :f]))


def test_the_nyquist_case_stays_finite():
    assert np.all(np.isfinite(R.expected("nyquist_low3")))
    assert R.coefficients(24000.0, R.SR, 1)[0] < -1e7                                 # the fp32 product lands past pi / 2
