"""tests/spectrum_reference.py against what it restates (Audio/AudioSynthesis.cpp:151-268), on the CPU: the table's truth against the direct
O( N^2 ) sum of the c2r's definition, the ignored imaginary parts of bins 0 and C, zeros where no harmonic is, the sd <= 0.001 branch, the
number of harmonics against a hand count, the single-precision stand-in's level, and the loop against the vectors the reference's own
WDL_Resampler made."""
import numpy as np
import pytest

import spectrum_reference as R

F32 = np.float32


def random_spectrum(p, seed):
    rng = np.random.default_rng(seed)
    _, _, B = R.sizes(p)
    return rng.uniform(0.0, 1.0, B).astype(F32), rng.uniform(0.0, 2 * np.pi, B).astype(F32)


@pytest.mark.parametrize("p", [6, 7, 8])
def test_truth_is_the_direct_sum(p):
    mag, theta = random_spectrum(p, p)
    truth, direct = R.table_truth(mag, theta), R.table_direct(mag, theta)
    assert truth.shape == (1 << p,)
    # fp64 both ways: N terms of size <= 2, each rounded at 2^-53
    assert np.max(np.abs(truth - direct)) <= (1 << p) * 2.0 * 2.0 ** -52


@pytest.mark.parametrize("p", [6, 8])
def test_imaginary_parts_of_bin_0_and_bin_c_are_ignored(p):
    mag, theta = random_spectrum(p, 40 + p)
    base = R.table_truth(mag, theta)
    # the same real parts with other imaginary parts: r' = r cos( theta ) / cos( theta' ) is not exact, so compare two spectra built in fp64
    N, C, B = R.sizes(p)
    import scipy.fft as sf
    X = mag.astype(np.float64) * np.exp(1j * theta.astype(np.float64))
    Y = X.copy()
    Y[0], Y[C] = X[0].real + 5.0j, X[C].real - 3.0j
    assert np.array_equal(sf.irfft(X, N), sf.irfft(Y, N))
    assert np.allclose(sf.irfft(X, N) * N, base, rtol=0, atol=0)
    # and the stand-in
    real = X.copy()
    real[0], real[C] = X[0].real, X[C].real
    a = sf.irfft(X.astype(np.complex64), N)
    b = sf.irfft(real.astype(np.complex64), N)
    assert np.array_equal(a, b)


def test_bins_without_a_harmonic_are_zero():
    for p, fp in ((10, 8), (13, 8), (8, 4)):
        harmonic, freq = R.bins(p, fp)
        mag = R.magnitudes(p, fp)
        assert harmonic[0] == 0 and np.any(harmonic == 0)
        assert np.all(mag[harmonic == 0] == 0) and np.all(mag[harmonic != 0] >= 0) and np.any(mag > 0)
        theta = R.phases(3, harmonic)
        assert np.all(theta[harmonic == 0] == 0) and np.all((theta >= 0) & (theta < 2 * np.pi + 1e-6))
        # bin_to_frequency divides by the number of bins, not by N: the last bin lies below 48000 by one bin's width
        B = freq.size
        assert freq[-1] == F32(F32(B - 1) * F32(48000.0)) / F32(B) and freq[1] == F32(48000.0) / F32(B)


def test_harmonics_round_half_away_from_zero():
    # p = 1 + log2( 375 * 2 ) is no power of two: take fundamental 2^4 and the bins of p = 6 ( B = 33 ): freq / 16 = b * 48000 / 33 / 16
    harmonic, freq = R.bins(6, 4)
    want = [int(np.floor(float(F32(f) / F32(16.0)) + 0.5)) for f in freq]
    assert harmonic.tolist() == want
    assert R.bins(6, 4)[0][1] == 91                   # 1454.5454 / 16 = 90.909


def test_the_flat_branch_where_the_spread_is_at_most_a_thousandth():
    p, fp = 10, 8
    harmonic, freq = R.bins(p, fp)
    scale = lambda h: F32(0.5)                        # noqa: E731
    flat = R.magnitudes(p, fp, spread=lambda h: F32(0.001), harmonic_scale=scale)
    on = harmonic != 0
    assert np.array_equal(flat[on], (freq[on] * F32(0.5)).astype(F32))          # r = x * harmonic_scale
    above = R.magnitudes(p, fp, spread=lambda h: F32(0.0011), harmonic_scale=scale)
    x = ((freq[on] - (F32(256.0) * harmonic[on].astype(F32))).astype(F32) / F32(0.0011)).astype(F32)
    assert np.array_equal(above[on], ((R.gaussian(x) / F32(0.0011)).astype(F32) * F32(0.5)).astype(F32))
    # one harmonic flat, the others not
    mixed = R.magnitudes(p, fp, spread=lambda h: F32(0.0005) if h == 3 else F32(h), harmonic_scale=scale)
    three = harmonic == 3
    assert np.array_equal(mixed[three], (freq[three] * F32(0.5)).astype(F32)) and np.any(three)


def test_num_harmonics_by_hand():
    assert R.num_harmonics(8) == 189                  # 48000 / 256 = 187.5 -> 188, + 1
    assert R.num_harmonics(7) == 376                  # 375 exactly, + 1
    assert R.num_harmonics(3) == 6001
    assert R.num_harmonics(16) == 2                   # 0.73 -> 1, + 1
    for p, fp in ((13, 8), (20, 8), (14, 3), (6, 4)):
        assert R.bins(p, fp)[0].max() <= R.num_harmonics(fp)


@pytest.mark.parametrize("p", [6, 13, 14, 16])
def test_the_stand_in_sits_at_single_precision(p):
    harmonic, _ = R.bins(p, min(8, p))
    mag = R.magnitudes(p, min(8, p))
    theta = R.phases(1000 + p, harmonic)
    truth, standin = R.table_truth(mag, theta), R.table_standin(mag, theta)
    err = np.max(np.abs(standin.astype(np.float64) - truth)) / np.max(np.abs(truth))
    print("p=%d: stand-in rel max %.3e" % (p, err))
    assert standin.dtype == F32 and 2.0 ** -27 < err < 2.0 ** -20


def test_jumps():
    assert [R.jump(c, 3, 13) for c in range(3)] == [0, 2730, 5461]
    assert [R.jump(c, 2, 20) for c in range(2)] == [0, 1 << 19]
    assert R.jump(0, 1, 22) == 0 and R.jump(6, 7, 22) == int(F32(6) / F32(7) * F32(1 << 22))


def test_golden_table_formula():
    t = R.golden_table(13)
    assert t.dtype == F32 and t.size == 8192 and t[0] == -0.5 and t[1] == F32(((2654435761 >> 8) / 2.0 ** 24) - 0.5)
    assert -0.5 <= t.min() and t.max() < 0.5


CASES = R.load_cases()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_loop_against_the_reference_made_output(c):
    assert np.array_equal(c["table"], R.golden_table(c["p"]))
    y = R.synth(c["table"], c["fundamental"], c["ch"], c["out_frames"], c["g"], c["freq"])
    assert np.array_equal(y.view(np.uint32), c["out"].view(np.uint32))
    blocks = R.synth_plan(c["out_frames"], c["fundamental"], c["g"], c["freq"])
    assert [b["wanted"] for b in blocks] == c["wanted"].tolist() and [b["num_out"] for b in blocks] == c["delivered"].tolist()
    # the three channels' jumps cross the period's end
    total_in = int(c["wanted"].sum())
    N = 1 << c["p"]
    assert any(R.jump(ch, c["ch"], c["p"]) + total_in > N for ch in range(c["ch"]))


def test_set_volume_leaves_the_last_frame_out():
    x = np.array([[0.25, -0.5, 0.125, 4.0]], F32)
    y, end = R.set_volume(x)
    assert end == 3 and np.array_equal(y, np.array([[0.5, -1.0, 0.25, 8.0]], F32))
    z, _ = R.set_volume(np.zeros((2, 5), F32))
    assert not np.any(z)
