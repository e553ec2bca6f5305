"""tests/comb_reference.py against closed forms (is the restatement of Audio::filter_comb right?), then its model of the device -- fp64
pointer jumping, u rounded once -- against its fp64 truth on the case table the GPU test uses.  No GPU.

Bounds, derived: fp64 jumping is exact to ~1e-15, so the model's u is the truth's rounded to fp32 once, | u - u_truth | <= 2^-23 | u_truth |
(1 ulp, which allows for the one rounding at 0.5); the output adds one rounding each of u[n], u[p], 1 - a, the two products and the sum:
| y - y_truth | <= 5 * 2^-24 * ( | a u[n] | + | ( 1 - a ) u[p] | )."""
import math

import numpy as np
import pytest

import comb_reference as R

F32, F64 = np.float32, np.float64
SR = R.SR


def impulse(n, ch=1):
    x = np.zeros((ch, n), F32)
    x[:, 0] = 1.0
    return x


def test_a_constant_delay_gives_powers_of_the_feedback():
    n, D, k = 400, 32, F32(0.8)
    p = R.links(n, SR, 750.0)                                      # d = ( 1 / 1500 ) * 48000 = 32 exactly in fp32
    assert np.array_equal(p[:D], np.full(D, -1)) and np.array_equal(p[D:], np.arange(n - D))
    for invert in (False, True):
        y, u = R.comb_fp32(impulse(n), SR, 750.0, k, 1.0, invert)
        want = np.zeros(n, F32)
        power = F32(1)
        for m in range(0, n, D):
            want[m] = power
            power = F32(power * (-k if invert else k))
        assert R.same_bits(u[0], want)
        assert R.same_bits(y[0], want)                             # wet_dry 1: y = u + 0 * u[p]
        y, _ = R.comb_fp32(impulse(n), SR, 750.0, k, 0.0, invert)   # wet_dry 0: y = f u[p]
        assert np.array_equal(y[0, D:], (-want if invert else want)[:-D]) and not y[0, :D].any()


def test_no_feedback_is_a_two_tap_mix():
    rng = np.random.default_rng(3)
    n = 3000
    x = rng.uniform(-1, 1, (2, n)).astype(F32)
    cutoff = rng.uniform(100.0, 24000.0, n).astype(F32)
    a = rng.uniform(0, 1, n).astype(F32)
    for invert in (False, True):
        f = F32(-1 if invert else 1)
        p = R.links(n, SR, cutoff)
        xp = np.where(p >= 0, x[:, np.maximum(p, 0)], F32(0))
        want = a * x + ((F32(1) - a) * f) * xp
        y, u = R.comb_fp32(x, SR, cutoff, 0.0, a, invert)
        assert R.same_bits(u, x) and R.same_bits(y, want)
        assert R.same_bits(R.comb_jump(x, SR, cutoff, 0.0, a, invert)[0], want)


def test_cutoff_1_hz_links_nothing_below_24000_frames():
    assert np.all(R.links(23999, SR, 1.0) == -1)
    assert np.all(R.links(23999, SR, 0.001) == -1)                 # clamped to 1
    p = R.links(24002, SR, 1.0)
    assert p[23999] == -1 and p[24000] == 0 and p[24001] == 1
    x = np.random.default_rng(4).uniform(-1, 1, (1, 5000)).astype(F32)
    y, u, rounds = R.comb_jump(x, SR, 1.0, 0.9, 1.0)
    assert rounds == 0 and R.same_bits(u, x) and R.same_bits(y, x)


def test_t_between_minus_one_and_zero_reads_frame_0():
    p = R.links(100, SR, 440.0)                                    # d = 54.54...
    assert np.all(p[:54] == -1) and p[54] == 0 and p[55] == 0 and p[56] == 1 and p[99] == 44
    _, u = R.comb_fp32(impulse(100), SR, 440.0, 0.5, 1.0)
    assert u[0, 54] == 0.5 and u[0, 55] == 0.5 and u[0, 56] == 0.0


def test_frame_0_at_nyquist_reads_zero():
    p = R.links(5, SR, 24000.0)                                    # d = 1: t = -1 at frame 0, no link; frame n reads n - 1
    assert list(p) == [-1, 0, 1, 2, 3]
    assert list(R.links(5, SR, 1.0e9)) == [-1, 0, 1, 2, 3]          # clamped to sample_rate / 2
    y, u = R.comb_fp32(np.ones((1, 5), F32), SR, 24000.0, 1.0, 1.0)
    assert list(u[0]) == [1, 2, 3, 4, 5]


def test_a_nan_cutoff_frame_has_no_link():
    cutoff = np.full(200, 24000.0, F32)
    cutoff[100] = np.nan
    p = R.links(200, SR, cutoff)
    assert p[100] == -1 and p[99] == 98 and p[101] == 100
    y, u = R.comb_fp32(np.ones((1, 200), F32), SR, cutoff, 1.0, 1.0)
    assert u[0, 99] == 100 and u[0, 100] == 1 and u[0, 101] == 2 and np.all(np.isfinite(y))


def test_the_links_are_int32_and_earlier_frames():
    for name in R.IDS:
        p = R.expected(name)["p"]
        assert p.dtype == np.int32 and np.all(p < np.arange(len(p))) and np.all(p >= -1)


@pytest.mark.parametrize("name", R.IDS)
def test_the_model_against_the_truth(name):
    c, e = R.case(name), R.expected(name)
    n = c["x"].shape[1]
    assert e["rounds"] <= math.ceil(math.log2(n)) if n > 1 else e["rounds"] == 0
    if name.startswith(("chain", "n4")):
        assert e["rounds"] == math.ceil(math.log2(n))              # one chain of n: every round is needed
    if name == "c1_no_links":
        assert e["rounds"] == 0
    u_err = np.abs(e["u"].astype(F64) - e["u64"])
    y_err = np.abs(e["y"].astype(F64) - e["y64"])
    loop_err = np.abs(e["y32"].astype(F64) - e["y64"])
    peak = np.abs(c["x"]).max()
    print("%s: rounds %d; model to truth: u %.3e ulp, y %.3e of its bound; fp32 loop to truth %.3e of the input peak"
          % (name, e["rounds"], (u_err / np.maximum(np.abs(e["u64"]) * 2.0 ** -23, 1e-300)).max(),
             (y_err / np.maximum(e["bound"], 1e-300)).max(), loop_err.max() / peak))
    assert np.all(u_err <= 2.0 ** -23 * np.abs(e["u64"]))
    assert np.all(y_err <= e["bound"])


def test_the_model_equals_the_fp32_loop_without_feedback_or_links():
    for name in ("c440_default", "sweep_k0", "c1_no_links", "n1"):
        e = R.expected(name)
        assert R.same_bits(e["y"], e["y32"]), name


def test_a_nan_sample_reaches_its_descendants_only():
    c, e = R.case("forest"), R.expected("forest")
    m = int(np.argmax(np.bincount(e["p"][e["p"] >= 0])))            # the frame most frames read
    x = c["x"].copy()
    x[1, m] = np.nan
    y, u, _ = R.comb_jump(x, *R.args(c)[1:])
    _, u32 = R.comb_fp32(x, *R.args(c)[1:])
    hit = R.descendants(e["p"], m)
    assert hit.sum() > 1 and not hit.all()
    assert np.array_equal(np.isfinite(u32[1]), ~hit)               # the reference's u is not finite exactly there
    assert np.array_equal(np.isfinite(u[1]), ~hit)                 # and so is the model's
    assert R.same_bits(u[0], e["u"][0]) and R.same_bits(u[2], e["u"][2]) and R.same_bits(u[:, ~hit], e["u"][:, ~hit])
    # a clean frame's parent is clean, so the clean frames' outputs are the twin's too
    assert R.same_bits(y[:, ~hit], e["y"][:, ~hit])
