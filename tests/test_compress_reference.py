"""The NumPy restatement of Audio::compress / set_volume (tests/compress_reference.py) against itself and against what a compressor
must do: the scan form equals the sequential loop, the static curve, the exact cases, set_volume's frame range.  No device."""
import numpy as np
import pytest

import compress_reference as R

F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("name", R.IDS)
def test_scan_form_equals_the_sequential_loop(name):
    c = R.case(name)
    n = c["x"].shape[1]
    side = c["x"] if c["side"] is None else c["side"]
    x_L, a_R, a_A = R.level(R.detector_input(side, n), c["sr"], dtype=F64, **c["params"])
    y_1, y_L = R.peak_detector(x_L, a_R, a_A, F64)
    for run in (1, 7, 64):
        s_1, s_L = R.peak_detector_scan(x_L, a_R, a_A, run)
        for got, want in ((s_1, y_1), (s_L, y_L)):
            _, rel_max = R.errors(got, want)
            assert rel_max <= 1e-12, (name, run, rel_max)


# the condition tests/test_gpu_compress.py puts on the device against the fp64 truth
TRUTH_FACTOR = 4.0
TRUTH_FLOOR = 8 * 2.0 ** -23


def _long_levels(name):
    c = R.long_case(name)
    return R.level(R.detector_input(c["x"], c["x"].shape[1]), c["sr"], dtype=F64, **c["params"])


def _gain_of(y_L):
    return R.pow10_of(-y_L / 20.0, F64)


def test_scan_form_equals_the_sequential_loop_past_one_pass_of_the_carry():
    """three passes of 256 run summaries at a run of 1, whole and window by window: both detectors, and the gain curve they give, which
    then meets what tests/test_gpu_compress.py asks of the device against the truth with room to spare"""
    name = "bursts_n131857_run1"
    x_L, a_R, a_A = _long_levels(name)
    y_1, y_L = R.peak_detector(x_L, a_R, a_A, F64)
    s_1, s_L = R.peak_detector_scan(x_L, a_R, a_A, 1)
    true_gain = R.long_expected(name, F64)[1]
    assert np.array_equal(_gain_of(y_L), true_gain)
    assert [w[0] for w in R.windows(x_L.size, 1)] == ["whole", "pass 0", "pass 1", "pass 1 head", "pass 2", "pass 2 head"]
    for label, lo, hi in R.windows(x_L.size, 1):
        for what, got, want in (("y_1", s_1, y_1), ("y_L", s_L, y_L), ("gain", _gain_of(s_L), true_gain)):
            rel_rms, rel_max = R.errors_over(got, want, lo, hi)
            print("%s %s %s: %.3e %.3e" % (name, label, what, rel_rms, rel_max))
            assert rel_rms <= 1e-12 and rel_max <= 1e-12, (label, what)


def test_a_state_lost_between_two_passes_misses_the_conditions_where_it_is_lost():
    """the carry kernel forgetting its state at the start of its second pass: both detectors start again from 0 at frame 65 536.  The
    gain over the first block of the pass misses the device's allowance against the truth 1e4 times over; 8192 frames on the bursts
    and the attack (1 ms there) have let go of it (1.4e-11 is left), which is why the windows are there"""
    name = "bursts_n131857_run1"
    cut = R.PASS_RUNS
    x_L, a_R, a_A = _long_levels(name)
    n = x_L.size
    broken = _gain_of(np.concatenate([R.peak_detector_scan(x_L[:cut], a_R[:cut], a_A[:cut], 1)[1], R.peak_detector_scan(x_L[cut:], a_R[cut:], a_A[cut:], 1)[1]]))
    want, truth = R.long_expected(name, F32)[1], R.long_expected(name, F64)[1]

    def ratio(lo, hi):
        t, own = R.errors_over(broken, truth, lo, hi), R.errors_over(want, truth, lo, hi)
        print("lost state, frames [%d, %d): vs truth %.3e %.3e (the fp32 loop: %.3e %.3e)" % ((lo, hi) + t + own))
        return t[0] / max(TRUTH_FACTOR * own[0], TRUTH_FLOOR), t[1] / max(TRUTH_FACTOR * own[1], TRUTH_FLOOR)
    assert min(ratio(cut, cut + 256)) >= 1e4
    assert max(ratio(0, n)) > 1.0 and max(ratio(cut, 2 * cut)) > 1.0
    assert max(ratio(cut + 8192, n)) <= 1.0


def test_composition_handles_the_identity_and_a_zero():
    step = (0.0, 0.0, -3.0)                                        # a = 0: the step forgets the state
    assert R.then1(R.IDENTITY1, step) == step
    assert R.then1(step, R.IDENTITY1) == step
    assert R.then1(R.IDENTITY1, R.IDENTITY1) == R.IDENTITY1        # 0 x -inf never formed
    assert not np.isnan(R.then1(R.IDENTITY1, (0.0, 1.0, -np.inf))[2])
    m = R.then1((0.5, 1.0, 2.0), (0.25, 3.0, 1.0))
    for y in (-10.0, 0.0, 10.0):
        assert R.apply1(m, y) == R.apply1((0.25, 3.0, 1.0), R.apply1((0.5, 1.0, 2.0), y))


@pytest.mark.parametrize("level_db,knee", [(-30.0, 0.0), (-8.0, 0.0), (-18.0, 6.0)], ids=["below", "above", "in_knee"])
def test_static_curve_of_the_fp32_loop(level_db, knee):
    """A positive DC input held for 50 release times: the gain settles at -( x_G - y_G ) dB"""
    sr, release = 8000.0, 0.1
    n = int(50 * release * sr)
    x = np.full((1, n), 10.0 ** (level_db / 20), F32)
    _, c = R.compress(x, sr, threshold=-20.0, ratio=3.0, attack=0.005, release=release, knee_width=knee)
    x_G = 20 * np.log10(float(x[0, 0]))
    over = x_G + 20.0
    if 2 * over <= -knee:
        y_G = x_G
    elif 2 * over >= knee:
        y_G = x_G + over * (1 / 3.0 - 1)
    else:
        y_G = x_G + (1 / 3.0 - 1) * (over + knee / 2) ** 2 / (2 * knee)
    if knee:
        assert -knee / 2 < over < knee / 2
    got_db = 20 * np.log10(float(c[-1]))
    print("%g dB in, knee %g: gain %.6f dB, static curve %.6f dB" % (level_db, knee, got_db, -(x_G - y_G)))
    assert abs(got_db + (x_G - y_G)) <= 1e-3
    if level_db == -30.0:
        assert got_db == 0.0
    else:
        assert got_db < -0.3


def test_ratio_one_and_all_negative_input_pass_unchanged():
    for name in ("ratio1", "negative"):
        out, c = R.expected(name)
        assert np.array_equal(out.view(np.uint32), R.case(name)["x"].view(np.uint32)), name
        assert np.all(c == 1.0)
    assert np.all(R.detector_input(R.case("negative")["x"], 100) == 0)          # no abs: a negative frame detects 0


def test_set_volume_ignores_the_last_frame():
    rng = np.random.default_rng(3)
    x = (0.25 * rng.uniform(-1, 1, (2, 1000))).astype(F32)
    x[1, 500] = -0.5                                                            # the largest magnitude in range
    x[0, -1] = 0.9                                                              # the peak, in the frame that is not looked at
    assert R.volume_end(1000, 48000.0) == 999
    assert R.get_max_sample_magnitude(x, 48000.0) == F32(0.5)
    y = R.set_volume(x, 48000.0, 0.8)
    assert np.array_equal(y, x * (F32(0.8) / F32(0.5)))
    assert y[0, -1] > 1.0
    assert np.array_equal(R.set_volume(np.zeros((2, 10), F32), 48000.0, 0.8), np.zeros((2, 10), F32))
    one = np.full((1, 1), 0.3, F32)                                             # a single frame: nothing is looked at, m = 0
    assert np.array_equal(R.set_volume(one, 48000.0, 0.8), one)
