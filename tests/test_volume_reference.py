"""tests/volume_reference.py against itself and against hand-computed anchors (no device, no library)."""
import math

import numpy as np

import volume_reference as V

F32 = np.float32


def test_ring_modulate_wraps_channels_and_frames():
    x = np.arange(1, 13, dtype=F32).reshape(3, 4)
    other = np.array([[2.0, 3.0, 5.0], [7.0, 11.0, 13.0]], F32)
    out = V.ring_modulate(x, other)
    assert out.tolist() == [[2, 6, 15, 8], [35, 66, 91, 56], [18, 30, 55, 24]]      # channel 2 reads channel 0 again; frame 3 reads frame 0


def test_fade_plan_hand_values():
    assert V.fade_plan(1000, 16, 16) == (16, 16)
    assert V.fade_plan(1000, -5, 7) == (0, 7) and V.fade_plan(1000, 7, -5) == (7, 0) and V.fade_plan(1000, -1, -1) == (0, 0)
    # 700 + 700 > 1000: scale = 1000.0f / 1400 = 0.714285731f; 700 * that = 500.000012 -> rounds to 500.0f in fp32 -> floor 500
    scale = F32(1000) / F32(1400)
    assert float(F32(700) * scale) == 500.0
    assert V.fade_plan(1000, 700, 700) == (500, 500)
    assert V.fade_plan(1000, 1000, 0) == (1000, 0) and V.fade_plan(1000, 1001, 0) == (int(np.floor(F32(1001) * (F32(1000) / F32(1001)))), 0)
    assert V.fade_plan(10, 3, 30) == (0, 9)                         # 10 / 33 * 3 = 0.909 -> 0; * 30 = 9.09 -> 9
    s, e = V.fade_plan(7, 5, 5)
    assert (s, e) == (3, 3) and s + e <= 7


def test_fade_frames_by_hand():
    x = np.ones((1, 6), F32)
    out = V.fade_frames(x, 2, 3, V.interp_linear)
    # start: frames 0, 1 times 0 / 2, 1 / 2; end: frames 5, 4, 3 times 0 / 3, 1 / 3, 2 / 3
    want = np.array([0.0, 0.5, 1.0, F32(2) / F32(3), F32(1) / F32(3), 0.0], F32)
    assert np.array_equal(out[0], want)
    # ranges that meet: 4 + 4 > 6 -> ( 3, 3 ): frames 0 .. 2 by the start, 3 .. 5 by the end, nothing twice
    out = V.fade_frames(np.ones((1, 6), F32), 4, 4, V.interp_linear)
    assert np.array_equal(out[0], np.array([0.0, F32(1) / F32(3), F32(2) / F32(3), F32(2) / F32(3), F32(1) / F32(3), 0.0], F32))
    assert np.array_equal(V.fade_frames(x, 0, 0, V.interp_sqrt), x)
    assert np.array_equal(V.fade_frames(x, -3, -4, V.interp_sqrt), x)


def test_waveforms_by_hand_and_against_the_truth():
    t = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.25, -0.25, -0.75, 7.5], F32)
    assert V.waveform(V.SQUARE, t).tolist() == [-1, -1, 1, 1, -1, -1, -1, -1, 1]           # fmod keeps the sign: a negative t0 is below 0.5
    assert V.waveform(V.SAW, t).tolist() == [-1, -0.5, 0, 0.5, -1, -0.5, -1.5, -2.5, 0]
    assert V.waveform(V.TRIANGLE, t).tolist() == [-1, 0, 1, 0, -1, 0, -2, -4, 1]
    rng = np.random.default_rng(1)
    t = (rng.uniform(-3, 3, 5000)).astype(F32)
    assert np.array_equal(V.waveform(V.SQUARE, t).astype(np.float64), V.waveform_truth(V.SQUARE, t))
    for kind in (V.SAW, V.TRIANGLE):             # fmod and the product by 2 or 4 are exact; the one addition rounds: half an ulp of a value below 8
        assert np.max(np.abs(V.waveform(kind, t) - V.waveform_truth(kind, t))) <= 2.0 ** -22
    assert np.max(np.abs(V.waveform(V.SINE, t) - V.waveform_truth(V.SINE, t))) < 6e-7      # pi2 * t0 rounds at 2^-22 near 2 pi
    assert abs(float(V.waveform(V.SINE, F32(0.25))) - 1.0) < 1e-7 and float(V.waveform(V.SINE, F32(-0.25))) < -0.999999


def test_moisture_anchors_and_error_scale():
    # s = 0 -> 0; power( 1 ) = 1 whatever the skew: s + a * s * sin( pi2 * fmod( pi2 * f, 1 ) )
    args = dict(sr_over=192000.0, sr=48000.0, n=100)
    assert V.moisture(F32(0), 0, amount=0.5, frequency=96.0, skew=4.0, **args) == 0
    one = V.moisture(F32(1), 0, amount=0.5, frequency=96.0, skew=4.0, **args)
    x = F32(V.PI2 * F32(96.0))
    assert one == F32(F32(1) + F32(0.5) * V.waveform(V.SINE, x))
    # s = -1: power = -1, the waveform (odd: fmod keeps the sign) changes sign and so does amount * s: -1 + 0.5 * w
    assert V.moisture(F32(-1), 0, amount=0.5, frequency=96.0, skew=4.0, **args) == F32(F32(-1) + F32(0.5) * V.waveform(V.SINE, x))
    rng = np.random.default_rng(2)
    s = rng.uniform(-1, 1, 200000).astype(F32)
    F = np.zeros(s.size, np.int64)
    for freq, lo, hi in ((96.0, 5e-5, 6e-4), (3.0, 1.5e-6, 2e-5)):      # the issue's orientation figures: 2.1e-4 and 6.2e-6
        e_ref = np.max(np.abs(V.moisture(s, F, amount=0.5, frequency=freq, skew=4.0, **args) - V.moisture_truth(s, F, amount=0.5, frequency=freq, skew=4.0, **args)))
        print("E_ref at frequency %g: %.3e" % (freq, e_ref))
        assert lo < e_ref < hi


def test_curve_index_and_its_clamp():
    idx, raw = V.curve_index(np.arange(9), 192000.0, 48000.0, 100)
    assert idx.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2]
    # a synthetic case where Frame( t * sr ) reaches n: F = 4 n exactly
    idx, raw = V.curve_index(np.array([399, 400]), 192000.0, 48000.0, 100)
    assert raw.tolist() == [99, 100] and idx.tolist() == [99, 99]
    curve = np.arange(100, dtype=F32) / F32(100)
    got = V.moisture(np.array([0.5, 0.5], F32), np.array([399, 400]), 192000.0, 48000.0, 100, curve, 3.0, 2.0)
    assert got[0] == got[1]                                            # both read curve[99]


def test_phases_by_hand():
    M = 8.0
    f = np.array([3.0, 3.0, 3.0, -7.0, -7.0, 20.0, 0.0], F32)
    # exclusive: 0, 3, 6, 9 % 8 = 1, -6 -> 2, -5 -> 3, 23 % 8 = 7
    assert (V.phases_truth(f, M) * M).tolist() == [0, 3, 6, 1, 2, 3, 7]
    assert (V.phases_fp32(f, M).astype(np.float64) * M).tolist() == [0, 3, 6, 1, 2, 3, 7]
    assert V.circular_distance(0.999, 0.001) < 0.0021 and V.circular_distance(0.25, 0.75) == 0.5


def test_fp32_phases_drift_past_the_fp64_bound():
    """the evidence that carrying the scan in fp64 is a gain: on the long sweep the reference's own arithmetic, grouped sequentially, sits farther
    from the exact modular sum than the 2^-23 of a cycle the device is held to"""
    n, M = 65536 + 257, 768000.0
    sweep = np.linspace(20.0, 20000.0, n).astype(F32)
    truth = V.phases_truth(sweep, M)
    d = V.circular_distance(V.phases_fp32(sweep, M), truth).max()
    print("fp32 sequential scan: %.3e of a cycle from the truth (bound for the device: %.3e)" % (d, 2.0 ** -23))
    assert d > 2.0 ** -23
    rounded = V.circular_distance(truth.astype(F32), truth).max()       # what one rounding of the truth costs
    assert rounded <= 2.0 ** -24


def test_energy_truth():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1e19, 0.0], [2e19, 0.0]], F32)
    e = V.energy_truth(x)
    assert e[0] == 25 and e[1] == 0
    assert np.isfinite(e[2]) and e[2] == F32(float(F32(1e19)) ** 2)     # 1e38 is below fp32's largest value, 3.4e38
    assert np.isinf(e[3])                                               # 4e38 is not
    assert V.ulp(1.0) == 2.0 ** -23


def test_adsr_anchors():
    a, d, s, r, lvl = 0.5, 0.25, 1.0, 0.25, 0.5
    g = lambda t, **k: float(V.adsr(t, a, d, s, r, lvl, **k))
    assert g(-0.001) == 0 and g(2.5) == 0
    assert g(0.0) == 0 and g(0.25) == 0.5 and g(0.25, a_exp=2.0) == 0.25
    assert g(0.5) == 1.0                                               # t == a: the decay's first value
    assert g(0.625) == 0.75 and g(0.75) == lvl                         # half way down; t == a + d: the sustain
    assert g(1.0) == lvl and g(1.75) == lvl                            # t == a + d + s: the release's first value, 1 * sLvl
    assert g(1.875) == 0.25 and g(1.875, r_exp=2.0) == 0.125
    assert g(2.0) == 0                                                 # t == a + d + s + r: not > the sum, not < it: the last branch
    assert g(2.0000002) == 0
    # the ar helper: no decay, no sustain, sustain level 1
    assert float(V.adsr(0.1, 0.2, 0, 0, 0.2, 1)) == 0.5 and float(V.adsr(0.2, 0.2, 0, 0, 0.2, 1)) == 1.0 and float(V.adsr(0.3, 0.2, 0, 0, 0.2, 1)) == F32(1) - F32(F32(F32(0.3) - F32(0.2)) / F32(0.2))


def test_white_noise_draw_is_in_range_and_seeded():
    a, b = V.white_noise_draw(7, 200), V.white_noise_draw(8, 200)
    assert np.array_equal(a, V.white_noise_draw(7, 200)) and not np.array_equal(a, b)
    assert a.min() >= -1 and a.max() <= 1 and abs(float(a.mean())) < 0.2


def test_hann_window_and_envelope_function():
    w, total = V.hann_window(F32(480.0))
    assert w.size == 480 and w[0] == 0 and abs(float(w[-1])) < 1e-6 and abs(float(w[240]) - 1.0) < 1e-4
    assert abs(float(total) - 239.5) < 1e-2                            # the integral of a Hann window over its n - 1 intervals
    assert V.hann_window(F32(0.5))[0].size == 0
    ys = np.array([1.0, 3.0, 2.0], F32)
    sr = 4.0
    assert V.envelope_function(ys, sr, 0.0) == 1 and V.envelope_function(ys, sr, 0.125) == 2 and V.envelope_function(ys, sr, 0.375) == 2.5
    assert V.envelope_function(ys, sr, 0.5) == 0 and V.envelope_function(ys, sr, -0.01) == 0      # x == size - 1 is outside


def test_synthesize_waveform_frames():
    assert V.synthesize_waveform_frames(0.5, 48000.0, 16) == (24000, 384000, 768000.0)
    assert V.synthesize_waveform_frames(0.5, 48000.0, 0) is None and V.synthesize_waveform_frames(0.0, 48000.0, 1) is None
    assert V.synthesize_waveform_frames(1.0, 0.0, 1) is None and V.synthesize_waveform_frames(1e-9, 48000.0, 4) is None


def test_mono_and_rectify():
    x = np.array([[1.0, -2.0, -0.0], [3.0, -4.0, 0.0]], F32)
    assert V.mono(x).tolist() == [2.0, -3.0, 0.0]
    r = V.rectify(np.array([-1.5, 2.0, -0.0, np.nan], F32))
    assert r[0] == 1.5 and r[1] == 2.0 and np.signbit(r[2]) and np.isnan(r[3])
    assert math.isclose(float(V.envelope_gain(F32(239.5))), math.pi / 2 / 239.5, rel_tol=1e-6)
