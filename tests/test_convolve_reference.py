"""The numpy restatement of Audio::convolve (tests/convolve_reference.py) and its fp64 truth, checked against np.convolve in float64 on
small shapes (no device)."""
import numpy as np
import pytest

import convolve_reference as R

SR = 48000.0


def _pair(ch, n, irch, m, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((ch, n)).astype(np.float32), rng.standard_normal((irch, m)).astype(np.float32)


def _direct(x, h):
    ch, n = x.shape
    irch, m = h.shape
    out = np.zeros((ch, n + m))
    for c in range(ch):
        out[c, : n + m - 1] = np.convolve(x[c].astype(np.float64), h[c % irch].astype(np.float64))
    return out


SHAPES = [(1, 1, 1, 1), (1, 1, 1, 7), (1, 7, 1, 1), (1, 100, 1, 37), (2, 256, 1, 255), (1, 3, 2, 300), (3, 129, 2, 64), (2, 300, 2, 299)]


@pytest.mark.parametrize("ch,n,irch,m", SHAPES)
def test_truth_is_np_convolve_with_channel_cycling(ch, n, irch, m):
    x, h = _pair(ch, n, irch, m, seed=n * 31 + m)
    t = R.truth(x, h)
    assert t.shape == (ch, n + m)
    np.testing.assert_array_equal(t, _direct(x, h))
    assert np.all(t[:, -1] == 0.0)


@pytest.mark.parametrize("ch,n,irch,m", SHAPES)
def test_restatement_is_within_fp32_round_off_of_np_convolve(ch, n, irch, m):
    x, h = _pair(ch, n, irch, m, seed=n * 7 + m)
    y = R.restatement(x, h, SR, normalize=False)
    assert y.dtype == np.float32 and y.shape == (ch, n + m)
    t = _direct(x, h)
    rel_rms, rel_max = R.errors(y, t)
    assert rel_rms < 1e-6 and rel_max < 1e-6, (rel_rms, rel_max)
    assert np.max(np.abs(y[:, -1])) < 1e-5 * np.max(np.abs(t))        # exactly 0 in exact arithmetic; round-off here


def test_large_truth_by_fft_matches_direct_sums():
    x, h = _pair(1, 3000, 1, 1500, seed=3)                              # n m above the direct-sum limit
    t = R.truth(x, h)
    d = _direct(x, h)
    assert np.max(np.abs(t - d)) < 1e-11 * np.max(np.abs(d))


def test_normalization_range_and_gain():
    # the scan stops before the last frame (clamp to N - 1), and the gain is the fp32 reciprocal of that max
    y = np.zeros((2, 10), np.float32)
    y[1, 3] = -0.5
    y[0, 9] = 4.0                                                        # the last frame is outside the range
    assert R.norm_end(10, SR) == 9
    assert R.max_magnitude(y, SR) == np.float32(0.5)
    z = R.normalized(y, SR)
    assert z[1, 3] == np.float32(-0.5) * (np.float32(1) / np.float32(0.5)) and z[0, 9] == np.float32(8.0)
    # the range as fp32 gives it: N / sr * sr is N or just below it, so the scan ends at N - 1 (and is empty for N = 1)
    for sr in (44100.0, 48000.0, 12345.678):
        assert all(R.norm_end(N, sr) == N - 1 for N in range(1, 5000))


def test_silence_normalizes_to_nan():
    x = np.zeros((1, 50), np.float32)
    h = np.ones((1, 5), np.float32)
    assert np.all(R.restatement(x, h, SR, normalize=False) == 0)
    assert np.all(np.isnan(R.restatement(x, h, SR, normalize=True)))
