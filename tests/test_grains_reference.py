"""tests/grains_reference.py pinned by cases worked by hand from the reference's sources (Audio/AudioCombination.cpp:102-170,
Audio/AudioSynthesis.cpp:310-374, Audio/AudioTemporal.cpp:190-234, Audio/AudioVolume.cpp:102-135, WindowFunctions.cpp:10-13).  No device."""
import itertools

import numpy as np

import grains_reference as R

F32 = np.float32


def _one_source_events(n_events, src_frames, channels=1):
    e = R.make_events(n_events)
    e["ch_stride"], e["src_frames"], e["channels"] = src_frames, src_frames, channels
    return e


def test_the_sum_order_is_the_index_order_and_it_shows():
    """1, 2^-24, 2^-23 on one frame: ( 1 + 2^-24 ) + 2^-23 = 1 + 2^-23 (the first sum is a tie and goes to even, 1), while both other groupings
    give 1 + 2^-22 (( 1 + 2^-23 ) + 2^-24 and 3 * 2^-24 + 1 are ties that go to the even 1 + 2^-22)"""
    sources = np.array([1.0, 2.0 ** -24, 2.0 ** -23, 7.0], F32)
    e = _one_source_events(3, 4)
    e["n"], e["o"] = [2, 2, 3], [5, 4, 3]                                      # frame 5: source frames 0, 1, 2; unsorted start frames
    got = R.mix32(e, sources, None, 1, 7, 48000.0)
    assert got[0, 5] == F32(1.0) + F32(2.0 ** -23)
    for order in itertools.permutations(range(3)):
        v = R.mix32(e, sources, None, 1, 7, 48000.0, order=order)[0, 5]
        if set(order[:2]) == {0, 1}:
            assert v == got[0, 5], order
        else:
            assert v == F32(1.0) + F32(2.0 ** -22), order
    assert R.mix64(e, sources, None, 1, 7, 48000.0)[0, 5] == 1.0 + 2.0 ** -24 + 2.0 ** -23
    # the other frames: 3: src[0]; 4: src[0] + src[1], a tie that goes to 1; 6: src[1]
    assert got[0, 3] == 1 and got[0, 4] == 1 and got[0, 6] == F32(2.0 ** -24)
    assert np.all(got[0, :3] == 0) and not np.any(np.signbit(got[0, :3]))


def test_a_lone_negative_zero_comes_out_positive():
    e = _one_source_events(1, 2)
    e["n"] = 2
    got = R.mix32(e, np.array([-0.0, -1.0], F32), None, 1, 2, 48000.0)
    assert got[0, 0] == 0 and not np.signbit(got[0, 0]) and got[0, 1] == -1


def test_fades_by_hand():
    """n = 8, sf = 2, ef = 3 over ones: sqrt( 0 / 2 ), sqrt( 1 / 2 ), 1, 1, 1, sqrt( 2 / 3 ), sqrt( 1 / 3 ), sqrt( 0 / 3 )"""
    e = _one_source_events(1, 8)
    e["n"], e["sf"], e["ef"] = 8, 2, 3
    got = R.mix32(e, np.ones(8, F32), None, 1, 8, 48000.0)[0]
    want = [0, np.sqrt(F32(0.5)), 1, 1, 1, np.sqrt(F32(2) / F32(3)), np.sqrt(F32(1) / F32(3)), 0]
    assert R.same_bits(got, np.array(want, F32))
    # fades that meet: sf + ef == n, no frame in both ramps
    e["sf"], e["ef"] = 5, 3
    got = R.mix32(e, np.ones(8, F32), None, 1, 8, 48000.0)[0]
    want = [np.sqrt(F32(k) / F32(5)) for k in range(5)] + [np.sqrt(F32(k) / F32(3)) for k in (2, 1, 0)]
    assert R.same_bits(got, np.array(want, F32))


def test_hann_by_hand():
    """n = 4 at any rate: x = 0, 1/4, 1/2, 3/4 -> 0, 1/2, 1, 1/2 up to the rounding of 2.0f * pi * x and of the double cos"""
    e = _one_source_events(1, 4)
    e["n"], e["flags"] = 4, R.HANN
    got = R.mix32(e, np.ones(4, F32), None, 1, 4, 48000.0)[0]
    assert got[0] == 0 and abs(got[1] - 0.5) < 1e-6 and abs(got[2] - 1) < 1e-6 and abs(got[3] - 0.5) < 1e-6
    a = F32(2.0) * F32(np.arccos(F32(-1.0))) * ((F32(1) * (F32(1) / F32(48000))) / (F32(4) / F32(48000)))
    assert got[1] == F32(0.5 * (1.0 - np.cos(np.float64(a))))
    assert np.allclose(R.mix64(e, np.ones(4, F32), None, 1, 4, 48000.0)[0], [0, 0.5, 1, 0.5], atol=1e-15)


def test_gains_and_channels():
    sources = np.arange(1, 9, dtype=F32)                                        # two channels of four frames
    e = _one_source_events(2, 4, channels=2)
    e["n"], e["o"] = [4, 3], [-1, 2]                                            # a negative start: frame 0 of the event is not heard
    e["gain"][0] = 0.5
    e["gain_offset"][1] = 1
    e["channels"][1] = 1                                                        # a mono source into a stereo output: channel 1 does not hear it
    gains = np.array([9, 2, 3, 4], F32)
    got = R.mix32(e, sources, gains, 2, R.out_frames(e), 48000.0)
    assert R.out_frames(e) == 5
    assert np.array_equal(got, np.array([[1.0, 1.5, 2.0 + 2, 6, 12], [3.0, 3.5, 4.0, 0, 0]], F32))


def test_cut_validation_by_hand():
    # truncation: 0.0100001 s at 48 kHz is frame 480; end <= start BEFORE the clamp
    assert R.cut_frames(100, 10, 10, 0, 0) == (0, 0, 0, 0)
    assert R.cut_frames(100, 20, 10, 0, 0) == (0, 0, 0, 0)
    assert R.cut_frames(100, 200, 300, 0, 0) == (0, 0, 0, 0)                   # after the clamp: both become 99, no frames
    assert R.cut_frames(100, -50, -10, 0, 0) == (0, 0, 0, 0)                   # both become 0
    assert R.cut_frames(100, -5, 10, 0, 0) == (0, 10, 0, 0)                    # a negative start is clamped
    assert R.cut_frames(100, 90, 500, 0, 0) == (90, 9, 0, 0)                   # the end is clamped to num_frames - 1
    assert R.cut_frames(100, 98, 99, 3, 3) == (98, 1, 0, 0)                    # n = 1: scale 1 / 6, both fades floor to 0
    # the rescale (AudioVolume.cpp:113-118): n = 10, 8 + 8 > 10: scale = 10 / 16, floor( 5 ) each
    assert R.cut_frames(100, 0, 10, 8, 8) == (0, 10, 5, 5)
    # 7 + 2 > 6: scale = 6 / 9 = 0.6666667f; 7 * that = 4.666667 -> 4; 2 * that = 1.3333334 -> 1
    assert R.cut_frames(100, 0, 6, 7, 2) == (0, 6, 4, 1)
    assert R.cut_frames(100, 0, 10, -3, 4) == (0, 10, 0, 4)                    # fades clamped at 0
    assert R.cut(48000, 48000.0, 0.0100001, 0.02, 0.001, 0.001) == (480, 480, 48, 48)
    for bad in (np.inf, -np.inf, np.nan, 1e30):
        assert R.cut(48000, 48000.0, 0.5, bad, 0.0, 0.0) == (0, 0, 0, 0), bad  # an unvoiced psola grain is 2.0f / 0 long
    assert R.cut(48000, 48000.0, 0.5, 0.6, np.nan, 0.0) == (0, 0, 0, 0)


def test_event_integration_by_hand():
    # the accumulator starts at 1.0f: the first event is at frame 0, and a rate of 0 yields only that one
    assert np.array_equal(R.events(1000, 48000.0, 0.0), [0])
    assert np.array_equal(R.events(1000, 48000.0, -5.0), [0])                  # the rate is clamped at 0
    # 12000 events per second at 48 kHz: a quarter per frame, exact in fp32.  The frame's share is added BEFORE the test (:332-333): frame 0
    # fires at 1.25 and keeps 0.25, which reaches 1 at frame 3; from there every fourth frame
    assert np.array_equal(R.events(20, 48000.0, 12000.0), [0, 3, 7, 11, 15, 19])
    # one event per frame and more: the floor is dropped, at most one event per frame
    assert np.array_equal(R.events(5, 48000.0, 3 * 48000.0), [0, 1, 2, 3, 4])
    # a rate that switches on: events only where the integral passes an integer
    rate = np.zeros(16, F32)
    rate[8:] = 24000.0
    assert np.array_equal(R.events(16, 48000.0, rate), [0, 9, 11, 13, 15])
    assert R.event_time(4800, 48000.0) == F32(0.1) and R.time_to_frame(R.event_time(4800, 48000.0), 48000.0) == 4800


def test_plan_by_hand():
    e = _one_source_events(4, 100)
    e["n"], e["o"] = [10, 0, 30, 5], [-5, 7, 8, 30]                             # tile 8: frames [0, 8), [8, 16), ...
    frames, first, last = R.plan(e, 8)
    assert frames == 38                                                         # max( o + n ); the empty event counts with its o alone
    assert list(first) == [0, 2, 2, 2, 2] and list(last) == [0, 2, 2, 3, 3]
    e["o"][1] = 50
    assert R.plan(e, 8)[0] == 50                                                # ... which can be what sets the length
    assert R.plan(R.make_events(0), 8)[0] == 0
