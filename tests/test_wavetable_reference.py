"""The Python restatement of flan::Wavetable (tests/wavetable_reference.py) against the vectors the reference's own WDL_Resampler made
(tests/golden/ref_made/wdl_wavetable.npz), and snap, starts and table_index on hand-made rows.  No device.

Also the condition tests/test_gpu_wavetable.py relies on when it demands the truth's rotations exactly: for every waveform of its resample
cases the truth's decision margin (the smallest |y| the zero-crossing search looks at) is at least 1e-4 of max |y|.  Measured: the
smallest relative margin is 2.8e-3 at W = 64, 3.5e-4 at W = 256 and 1.4e-3 at W = 2048; the single-precision stand-in chooses the truth's
rotation every time, with relative-max error <= 5.1e-7 (recorded, not a bound)."""
import numpy as np
import pytest

import wavetable_reference as R

F32 = np.float32
CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)                     # the run planner's cases (wdl_wavetable_runs.npz): held to the same here
RUN_IDS = [c["name"] for c in RUN_CASES]


@pytest.mark.parametrize("c", CASES + RUN_CASES, ids=IDS + RUN_IDS)
def test_the_restatement_equals_the_reference_made_output(c):
    blocks = R.synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    assert len(blocks) == c["blocks"]
    assert np.array_equal([b["wanted"] for b in blocks], c["wanted"])
    assert np.array_equal([b["num_out"] for b in blocks], c["delivered"])           # a block ends where its input does, not after g frames
    first = np.array([b["first_out"] for b in blocks])
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(c["delivered"])[:-1]]))
    y = R.synth(c["table"], c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], c["index"][:, first], c["smooth"], blocks=blocks)
    assert np.array_equal(y.view(np.uint32), c["out"].view(np.uint32))


def test_the_fixture_holds_the_cases_the_branches_need():
    by = dict(zip(IDS, CASES))
    shape = lambda c: R.WDL.table_shape(max(float(c["freq"][0]), 1.0), c["sr"] / c["W"], max(float(c["freq"][0]), 1.0) / (c["sr"] / c["W"]))   # noqa: E731
    assert shape(by["f750_ideal1"])[1:] == (1, True)
    assert shape(by["f375_ideal2"])[1:] == (2, True)
    assert shape(by["f1500_ideal_lp"])[0] < 1.0 and shape(by["f1500_ideal_lp"])[2]
    assert not shape(by["f1027p5"])[2]
    assert by["f100"]["wanted"][1:].max() <= 9                               # 9 input samples per block: a tap window spans 7 blocks' blends
    assert by["f0"]["delivered"].max() > 2048 and np.array_equal(by["f0"]["wanted"], by["fneg5"]["wanted"])      # the 1 Hz clamp
    assert by["plus17"]["delivered"][-1] < 48 and by["frames20"]["blocks"] == 1
    assert np.all(by["rneg"]["index"] == 0) and np.array_equal(by["rbig"]["index"][:, 0], [4, 2])              # the clamps of the table index
    assert not by["unsmooth"]["smooth"] and by["w2048"]["W"] == 2048


# ---------------------------------------------------------------------------------------------------------------
# snap

def ramp(n, crossing):
    """negative before `crossing`, positive from it on"""
    return (np.arange(n) - crossing + 0.5).astype(F32) / n


def test_snap_finds_a_crossing_on_the_left():
    row = ramp(100, 47)                                                      # frame 50 is above; the first frame below, going left, is 46
    assert R.snap(row, 50, 0.0, 10) == 47                                    # left + 1


def test_snap_finds_a_crossing_on_the_right():
    row = -ramp(100, 53)                                                     # frame 50 is above; frame 53 is the first below
    assert R.snap(row, 50, 0.0, 10) == 53


def test_snap_prefers_left_at_equal_distance_and_keeps_the_asymmetric_limits():
    row = np.ones(100, F32)
    row[45] = row[55] = -1
    assert R.snap(row, 50, 0.0, 10) == 46                                    # the left frame is tested first
    row = np.ones(100, F32)
    row[40] = row[60] = -1
    assert R.snap(row, 50, 0.0, 10) == 41                                    # left: >= limit; right: < limit, so frame 60 is never looked at
    row[40] = 1
    assert R.snap(row, 50, 0.0, 10) == 50                                    # ... and the fallback finds nothing nearer than the frame itself


def test_snap_falls_back_to_the_nearest_sample():
    row = np.full(100, 0.5, F32)
    row[53] = 0.1                                                            # no crossing: | data - height | ( 1 + | f - frame | / distance ) is least here
    assert R.snap(row, 50, 0.0, 10) == 53
    row[48] = 0.1                                                            # nearer to the frame: preferred
    assert R.snap(row, 50, 0.0, 10) == 48


def test_snap_with_distance_zero_returns_the_frame():
    row = ramp(100, 50)
    assert R.snap(row, 50, 0.0, 0) == 50
    assert R.snap(row, 0, 0.0, 0) == 0
    assert R.snap(row, 99, 0.0, 0) == 99


def test_snap_at_the_rows_edges():
    row = ramp(100, 3)
    assert R.snap(row, 0, 0.0, 10) == 3                                      # frame 0 is below; nothing to its left
    assert R.snap(-row, 99, 0.0, 200) == 3                                   # the limits are clamped to the row


# ---------------------------------------------------------------------------------------------------------------
# starts

def sine_row(n, period, phase=0.3):
    return np.sin(2 * np.pi * (np.arange(n) + phase) / period).astype(F32)


def test_starts_fixed_frames_without_snapping():
    row = sine_row(1000, 100)
    assert R.starts(row, None, 0, R.SNAP_NONE, R.PITCH_NONE, 0.3, 256).tolist() == [0, 256, 512, 768]          # 768 + 256 >= 1000 ends the walk
    assert R.starts(row, None, 0, R.SNAP_NONE, R.PITCH_NONE, 0.3, 1000).tolist() == [0]                        # a start at frame 0 alone: 0 + 1000 >= 1000
    assert R.starts(row, None, 0, R.SNAP_NONE, R.PITCH_NONE, 0.3, 999).tolist() == [0, 999]                    # >=, not >


def test_starts_snap_to_rising_zero_crossings():
    row = sine_row(1000, 100)                                                # upward crossings at 99.7, 199.7, ...
    got = R.starts(row, None, 97, R.SNAP_ZERO, R.PITCH_GLOBAL, 0.3, 256)
    # frame 0 is above and no crossing lies within Frame( 0.3f * 97 ) = 29 frames: the fallback keeps it; then every guess of + 97 snaps to
    # the crossing three frames on; the last guess, 997, finds none before the row ends and falls back to the frame nearest to zero
    assert got.tolist() == [0, 100, 200, 300, 400, 500, 600, 700, 800, 900, 999]
    for s in got[1:-1]:
        assert row[s] > 0 and row[s - 1] <= 0


def test_starts_level_mode_snaps_to_the_previous_starts_height():
    row = sine_row(1000, 100)
    got = R.starts(row, None, 98, R.SNAP_LEVEL, R.PITCH_GLOBAL, 0.3, 256)
    # the first start looks for the level of frame 0 itself: frame 1 is the first above it; every later start is the first frame above the
    # level of the start before it, one period and one frame on
    assert got.tolist() == [1, 102, 203, 304, 405, 506, 607, 708, 809, 910]


def test_starts_with_a_global_wavelength_of_minus_one():
    row = sine_row(1000, 100)
    # Frame( get_average_wavelength ) = -1 in Local mode: the first snap has max_snap Frame( 0.3f * -1 ) = 0, locals of 0 fall to the fixed frame
    got = R.starts(row, np.zeros(8, F32), -1, R.SNAP_ZERO, R.PITCH_LOCAL, 0.3, 250)
    assert got[0] == 0
    assert np.all(np.abs(np.diff(got) - 250) <= 75)


def test_starts_local_wavelengths_fall_back_to_the_global_then_the_fixed_frame():
    row = sine_row(2000, 100)
    locals_ = np.array([100.7, 0, 0, 100.2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], F32)          # truncated: 100; one per 128 frames
    got = R.starts(row, locals_, 150, R.SNAP_NONE, R.PITCH_LOCAL, 0.3, 40)
    assert got.tolist()[:5] == [0, 100, 200, 350, 500]                       # local 100 twice (frames 0, 100 -> index 0), then the global 150
    got = R.starts(row, locals_, 0, R.SNAP_NONE, R.PITCH_LOCAL, 0.3, 40)
    assert got.tolist()[:6] == [0, 100, 200, 240, 280, 320]                  # no global: the fixed frame


def test_starts_stop_where_the_local_wavelengths_end_or_the_buffer_does():
    row = sine_row(2000, 100)
    got = R.starts(row, np.full(3, 120.0, F32), 0, R.SNAP_NONE, R.PITCH_LOCAL, 0.3, 40)
    assert got.tolist() == [0, 120, 240, 360, 480]                           # 360 / 128 = 2 is the last entry; 480 / 128 = 3 is past the end
    got = R.starts(row, np.full(100, 900.0, F32), 0, R.SNAP_NONE, R.PITCH_LOCAL, 0.3, 40)
    assert got.tolist() == [0, 900, 1800]                                    # 1800 + 900 >= 2000


# ---------------------------------------------------------------------------------------------------------------
# table index

def test_table_index():
    s = [10, 110, 310, 610]
    assert R.table_index(s, 1000, 0.0) == 0 and R.table_index(s, 1000, -0.5) == 0
    assert R.table_index(s, 1000, 0.005) == 0                                # frame 5 lies before the first start: upper_bound is the first
    assert R.table_index(s, 1000, 0.06) == F32(0.5)                          # frame 60 of [10, 110)
    assert R.table_index(s, 1000, 0.21) == F32(1.5)
    assert R.table_index(s, 1000, 0.11) == 1                                 # a start itself belongs to the waveform it begins
    assert R.table_index(s, 1000, 0.61) == 3 and R.table_index(s, 1000, 0.9) == 3 and R.table_index(s, 1000, 1.0) == 3
    assert R.table_index(s, 1000, 1.5) == 3                                  # source_frame > num_source_frames
    assert R.table_index(s, 1000, 0.0604) == F32(F32(50) / F32(100))         # Frame( 60.4 ) = 60: truncation
    assert R.table_index([0], 1000, 0.5) == 0


# ---------------------------------------------------------------------------------------------------------------
# the resample cases

@pytest.mark.parametrize("W", R.RESAMPLE_W)
def test_resample_cases_have_the_margin_the_gpu_test_relies_on(W):
    audio, starts = R.resample_case(W)
    lengths = sorted(set(int(b) - int(a) for s in starts for a, b in zip(s[:-1], s[1:])))
    assert set(R.resample_lengths(W)) <= set(lengths) and 0 in lengths
    assert len(set(len(s) for s in starts)) > 1                              # a ragged table
    truth, rot, margins, maxima = R.build_table(audio.astype(np.float64), starts, W)
    rel = margins / maxima
    print("W=%d: smallest relative decision margin %.3e" % (W, rel.min()))
    assert np.all(margins >= 1e-4 * maxima)
    standin, rot_s, _, _ = R.build_table(audio, starts, W, R.resample_standin)
    assert np.array_equal(rot, rot_s)
    worst = max(np.max(np.abs(standin[c, w * W:(w + 1) * W] - truth[c, w * W:(w + 1) * W])) / np.max(np.abs(truth[c, w * W:(w + 1) * W]))
                for c, s in enumerate(starts) for w in range(len(s) - 1) if s[w + 1] > s[w])
    print("W=%d: the stand-in's relative-max error %.3e" % (W, worst))
    for c, s in enumerate(starts):                                           # the zero slots: a channel's last, those of a shorter channel, n = 0
        for w in range(truth.shape[1] // W):
            if w + 1 >= len(s) or s[w + 1] <= s[w]:
                assert not np.any(truth[c, w * W:(w + 1) * W])


def test_resample_truth_on_shapes_with_a_known_answer():
    W = 64
    y, zc, _, _ = R.resample_truth(np.array([0.25]), W)                     # n = 1: a constant
    assert np.allclose(y, 0.25) and zc == 0
    x = np.sin(2 * np.pi * (np.arange(32) + 0.5) / 32)                       # one period over n = 32: the same period over W = 64
    y, zc, _, _ = R.resample_truth(x, W)
    assert np.allclose(y, np.sin(2 * np.pi * (np.arange(W) + zc + 1.0) / W), atol=1e-12)
    x = np.random.default_rng(3).standard_normal(130)                        # n > W: bins above W/2 are dropped, bin W/2 keeps its real part
    X = np.fft.rfft(x)
    Z = X[:W // 2 + 1].copy()
    Z[-1] = Z[-1].real
    y, zc, _, _ = R.resample_truth(x, W)
    assert np.allclose(np.roll(y, zc) * 130, np.fft.irfft(Z, W) * W, atol=1e-10)


# ---------------------------------------------------------------------------------------------------------------
# the edits

def test_edits_on_a_small_table():
    W = 8
    t = np.array([[1, 2, 3, 4, 4, 3, 2, 1, 0.0001, 0, 0, 0, 0, 0, 0, 0.0002]], F32)
    n = R.normalize(t, W)
    assert np.array_equal(n[0, :W], t[0, :W] / F32(4)) and np.array_equal(n[0, W:], t[0, W:])       # below 0.001: untouched
    assert np.allclose(R.remove_dc(t, W)[0, :W].sum(), 0)
    assert np.array_equal(R.add_fades(t, W, 1), t.astype(np.float64))
    f = R.add_fades(t, W, 2)
    assert np.array_equal(f[0, 1:W - 1], t[0, 1:W - 1]) and np.isclose(f[0, 0], np.sin(np.pi / 4)) and np.isclose(f[0, W - 1], np.sin(np.pi / 4))
    j = R.remove_jumps(np.array([[1, 2, 3, 4, 4, 3, 2, 3]], F32), W, 2)      # mid = 2
    assert np.isclose(j[0, 0], (1 - 2) * np.sin(np.pi / 4) + 2) and np.isclose(j[0, W - 1], (3 - 2) * np.sin(np.pi / 4) + 2)
