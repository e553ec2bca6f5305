"""tests/multinotch_reference.py against what it must be (is the restatement of the multinotches right?): the state-space form against the
fp64 loop, the closed forms at feedback 0 and wet_dry 1, the all-pass property, invert, the notch count, and the conditioning of every case of
the table.  No GPU, no flan_amd."""
import numpy as np
import pytest

import multinotch_reference as R

F32, F64 = np.float32, np.float64
SR = 48000.0


def noise(ch, n, seed=7):
    return np.random.default_rng(seed).normal(0.0, 0.3, (ch, n)).astype(F32)


def impulse(n):
    x = np.zeros((1, n), F32)
    x[0, 0] = 1.0
    return x


def allpass_cascade(x, sr, kind, order, cutoff, damping, dtype):
    """the sections alone, no feedback path: `order` all-passes in turn, from rows()' g"""
    g_row, R_row, _, _ = R.rows(x.shape[1], sr, cutoff, damping, 0.0, 0.0, False)
    T = dtype
    y = x.astype(T)
    for _ in range(order):
        s1, s2 = np.zeros(x.shape[0], T), np.zeros(x.shape[0], T)
        out = np.zeros_like(y)
        for f in range(x.shape[1]):
            g, Rf, u = T(g_row[f]), T(R_row[f]), y[:, f]
            if kind == R.ONE_POLE:
                v = g / (T(1) + g) * (u - s1)
                lp = v + s1
                s1 = lp + v
                out[:, f] = lp - (u - lp)
            else:
                d = T(1) / (T(1) + T(2) * Rf * g + g * g)
                hp = (u - (T(2) * Rf + g) * s1 - s2) * d
                v1 = g * hp
                bp = v1 + s1
                s1 = bp + v1
                v2 = g * bp
                lp = v2 + s2
                s2 = lp + v2
                out[:, f] = (lp - bp * T(2) * Rf) + hp
        y = out
    return y


@pytest.mark.parametrize("kind,order", [(R.ONE_POLE, 1), (R.ONE_POLE, 3), (R.ONE_POLE, 8), (R.ONE_POLE, 16),
                                        (R.TWO_POLE, 1), (R.TWO_POLE, 3), (R.TWO_POLE, 8)])
@pytest.mark.parametrize("invert", [False, True])
def test_the_state_space_form_is_the_fp64_loop(kind, order, invert):
    n = 300
    x = noise(2, n)
    cutoff, damping, feedback, wet_dry = R.curves(n)
    for par in ((1000.0, 0.7, 0.9, 0.5), (cutoff, damping, feedback, wet_dry), (cutoff, 0.3, -0.9, wet_dry)):
        want, _ = R.multinotch(x, SR, kind, order, *par, invert, dtype=F64)
        got = R.multinotch_state_space(x, SR, kind, order, *par, invert)
        assert np.max(np.abs(got - want)) <= 1e-12 * max(1.0, np.max(np.abs(want))), (kind, order, invert)


@pytest.mark.parametrize("kind,order", [(R.ONE_POLE, 1), (R.ONE_POLE, 5), (R.TWO_POLE, 1), (R.TWO_POLE, 4)])
def test_without_feedback_x_bar_is_the_input_and_the_output_the_mixed_all_pass(kind, order):
    n = 400
    x = noise(2, n)
    cutoff, damping, _, wet_dry = R.curves(n)
    for invert in (False, True):
        y, xb = R.multinotch(x, SR, kind, order, cutoff, damping, 0.0, wet_dry, invert, dtype=F32)
        assert R.same_bits(xb, x)
        ap = allpass_cascade(x, SR, kind, order, cutoff, damping, F32)
        want = wet_dry * x + (F32(1) - wet_dry) * (ap * F32(-1 if invert else 1))
        assert R.same_bits(y, want.astype(F32))


@pytest.mark.parametrize("kind,order", [(R.ONE_POLE, 1), (R.ONE_POLE, 8), (R.ONE_POLE, 16), (R.TWO_POLE, 1), (R.TWO_POLE, 8)])
def test_the_cascade_without_feedback_is_all_pass(kind, order):
    """wet_dry 0, feedback 0: the impulse response has unit energy"""
    y, _ = R.multinotch(impulse(6000), SR, kind, order, 1000.0, 0.7, 0.0, 0.0, False, dtype=F64)
    assert abs(float(np.sum(y * y)) - 1.0) <= 1e-6


@pytest.mark.parametrize("kind", [R.ONE_POLE, R.TWO_POLE])
def test_wet_is_x_bar(kind):
    n = 300
    x = noise(2, n)
    cutoff, damping, feedback, _ = R.curves(n)
    y, xb = R.multinotch(x, SR, kind, 3, cutoff, damping, feedback, 1.0, True, dtype=F32)
    assert R.same_bits(y, xb) and not R.same_bits(xb, x)


@pytest.mark.parametrize("kind", [R.ONE_POLE, R.TWO_POLE])
def test_invert_flips_the_feedback_and_the_dry_path(kind):
    """inv multiplies k and y_bar: x_bar( invert, k ) = x_bar( k -> -k ), and at wet_dry 0 the output is the negative"""
    n = 300
    x = noise(2, n)
    cutoff, damping, feedback, _ = R.curves(n)
    y_i, xb_i = R.multinotch(x, SR, kind, 4, cutoff, damping, feedback, 0.0, True, dtype=F32)
    y_n, xb_n = R.multinotch(x, SR, kind, 4, cutoff, damping, -feedback, 0.0, False, dtype=F32)
    assert R.same_bits(xb_i, xb_n) and R.same_bits(y_i, -y_n)
    y_p, _ = R.multinotch(x, SR, kind, 4, cutoff, damping, feedback, 0.0, False, dtype=F32)
    assert not R.same_bits(y_p, y_n)


@pytest.mark.parametrize("pairs", [1, 2, 3])
def test_a_1pole_cascade_of_2n_sections_has_n_notches(pairs):
    """wet_dry 0.5 without feedback is ( x + allpass^2n( x ) ) / 2: the phase runs through 2 n pi up to Nyquist, a null at every odd multiple of pi"""
    y, _ = R.multinotch(impulse(16384), SR, R.ONE_POLE, 2 * pairs, 2000.0, 1.0, 0.0, 0.5, False, dtype=F64)
    mag = np.abs(np.fft.rfft(y[0]))
    inner = mag[1:-1]
    nulls = np.flatnonzero((inner < mag[:-2]) & (inner < mag[2:]) & (inner < 0.02))
    assert len(nulls) == pairs, nulls
    assert float(np.max(mag)) <= 1.0 + 1e-9


@pytest.mark.parametrize("name", R.IDS)
def test_every_case_is_well_conditioned(name):
    """the fp32 loop within 1e-4 relative rms of the truth: what makes the truth criterion on the device mean something"""
    c, e = R.case(name), R.expected(name)
    assert np.all(np.isfinite(e["y32"])) and np.all(np.isfinite(e["y64"]))
    rms, _ = R.errors(e["y32"], e["y64"])
    scale = float(np.sqrt(np.mean(e["y64"] ** 2)))
    print("%s: fp32 loop vs truth rel rms %.3e" % (name, rms / scale if scale else 0.0))
    assert scale > 0.0 and rms <= 1e-4 * scale
    kind, order, n, ch, sr, invert, sig, params, run = R.CASES[name]
    assert c["x"].shape == (ch, n) and abs(np.max(np.abs(np.asarray(c["feedback"])))) <= 0.95
    assert 0.2 <= np.min(c["damping"]) and np.max(c["damping"]) <= 1.5


def test_the_table_covers_what_it_must():
    col = lambda i: {v[i] for v in R.CASES.values()}                    # noqa: E731
    assert {1, 3, 255, 256, 257, 1000, 8192, 9001} == col(2) and {1, 3} == col(3) and {48000.0, 44100.0} == col(4)
    assert {o for k, o, *_ in R.CASES.values() if k == R.ONE_POLE} == {1, 2, 3, 8, 16}
    assert {o for k, o, *_ in R.CASES.values() if k == R.TWO_POLE} == {1, 3, 4, 8}
    assert col(5) == {False, True} and col(6) == {"noise", "impulse", "step"} and col(7) == {"scalars", "curves"}
    assert all(v[8] == (0 if v[2] > 1000 else 1) for v in R.CASES.values())
    assert all(R.CASES[name][6] == "noise" for name in R.LONG_NOISE)
