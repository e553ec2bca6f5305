"""The NumPy restatement of the phase-difference network and the methods over it (tests/halfband_reference.py) against what the issue
pins: the poles, the all-pass and 90 degree properties of the fp64 restatement, the algebra halfband.hip scans by, and what
shift_frequency does to a sine."""
import numpy as np

import filter_reference as R1
import halfband_reference as R

F32, F64 = np.float32, np.float64
# phase_diff_network_pole_design( 20, 5, 22000 ): the FIRST output's cascade has the odd-indexed poles
FIRST = (27.732187, 87.724472, 230.03622, 606.9425, 1626.9309, 4375.6157, 11651.303, 30485.66, 83059.594, 499969.59)
SECOND = (8.6857805, 52.283253, 142.44815, 372.71591, 992.46051, 2669.2136, 7154.9214, 18878.01, 49503.016, 156591.53)


def ulps(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def test_the_poles_are_the_pinned_ones():
    first, second = R.poles()
    assert first.dtype == F32 and second.dtype == F32 and first.shape == (10,) and second.shape == (10,)
    assert np.all(ulps(first, np.array(FIRST, F32)) <= 1), first
    assert np.all(ulps(second, np.array(SECOND, F32)) <= 1), second
    # no prewarp, no clamp: g runs from 5.7e-4 to 32.7 at 48 kHz
    g = np.stack([first, second]) * (R.PI / F32(48000))
    assert abs(g.min() - 5.7e-4) < 1e-5 and abs(g.max() - 32.7) < 0.05


def test_the_cascades_are_all_pass_and_90_degrees_apart():
    hz = np.geomspace(50.0, 15000.0, 2000)
    H = R.response(48000.0, hz)
    assert np.max(np.abs(np.abs(H) - 1.0)) <= 1e-12
    lead = np.degrees(np.angle(H[0] / H[1]))
    print("the first leads the second by %.4f ... %.4f degrees" % (lead.min(), lead.max()))
    assert np.all(np.abs(lead - 90.0) <= 0.02)
    # the response is the loop's: the fp64 loop's impulse response, transformed, at frequencies it has rung out for
    n = 1 << 15
    x = np.zeros((1, n), F32)
    x[0, 0] = 1.0
    first, second = R.network(x, 48000.0, F64)
    for h, want in ((first[0], H[0]), (second[0], H[1])):
        got = np.array([np.sum(h * np.exp(-2j * np.pi * f / 48000.0 * np.arange(n))) for f in hz[::400]])
        assert np.max(np.abs(got - want[::400])) <= 0.02          # what is left of the slowest section's tail after 0.68 s


def test_a_cascade_is_one_linear_system_with_a_lower_triangular_matrix():
    """halfband.hip's algebra: s' = A s + b x, a run of L frames is A^L s + r with r the run's response from 0"""
    for sr in (44100.0, 48000.0):
        for G in R.coefficients(sr):
            A, b, c, d = R.state_space(G)
            assert np.array_equal(A, np.tril(A)) and np.all(np.abs(np.diag(A)) < 1.0)
            x = R.noise(1, 300, 5)
            y = R.cascade_rows(x, G[None], F64)[0]
            s, out = np.zeros(R.K), []
            states = [s]
            for v in x[0].astype(F64):
                out.append(c @ s + d * v)
                s = A @ s + b * v
                states.append(s)
            assert np.max(np.abs(np.array(out) - y)) <= 1e-13
            # the state after frames 100 ... 299 from the state after frame 99: a power of A and the response from 0
            r = np.zeros(R.K)
            for v in x[0, 100:].astype(F64):
                r = A @ r + b * v
            assert np.max(np.abs(np.linalg.matrix_power(A, 200) @ states[100] + r - states[300])) <= 1e-13


def test_the_fp32_loop_is_close_to_the_truth():
    x = R.noise(1, 4000, 3)
    rms, peak = R.scale(x)
    for got, truth in zip(R.network(x, 48000.0, F32), R.network(x, 48000.0, F64)):
        assert got.dtype == F32 and truth.dtype == F64
        rel_rms, rel_max = R.errors(got, truth, rms, peak)
        assert 1e-8 < rel_rms < 2e-6 and rel_max < 1e-5


def test_shift_curves_are_the_reference_s_fp32_arithmetic():
    sr = 48000.0
    shift = np.array([0.0, 100.0, -50.0, 250.0, -0.0, 1e-3], F32)
    lp, hp, phase = R.shift_curves(shift, sr, 30.0)
    assert lp.tolist() == [23000.0, 22900.0, 23000.0, 22750.0, 23000.0, float(F32(23000.0) - F32(1e-3))]
    assert hp.tolist() == [30.0, 30.0, 80.0, 30.0, 30.0, 30.0]
    acc, want = F32(0), []
    for s in shift:
        want.append(acc)
        acc = F32(acc + F32(F32(s * R.PI2) / F32(sr)))
    assert phase.dtype == F32 and phase.tolist() == [float(v) for v in want]


def test_shift_frequency_moves_a_sine():
    n, sr = 9600, 48000.0
    x = R1.sine(1, n, 1000.0)
    y = R.shift_frequency(x, sr, np.full(n, 250.0, F32), dtype=F32)[0]
    half = y[n // 2:].astype(F64)
    spec = np.abs(np.fft.rfft(half * np.hanning(len(half))))
    assert int(np.argmax(spec)) * sr / len(half) == 1250.0
    assert spec[int(750 * len(half) / sr)] < 0.01 * spec.max()
