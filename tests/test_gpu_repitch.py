"""Audio::repitch on the MI355X (flan_amd/csrc/repitch.hip) against the vectors the reference's own WDL_Resampler made
(tests/golden/ref_made/wdl_repitch.npz) and against the Python restatement (tests/repitch_reference.py).
Bounds: DESIGN.md 4.13 lists the measured values they are set from (<= 30 % above)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import repitch_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
# against the reference-made outputs / the restatement: relative rms error, and max abs error / max |y|
REL_RMS_BOUND = 2.7e-9          # measured at most 2.142e-9 (random shape 16: 2 ch x 2693, g = 6000, against the restatement)
REL_MAX_BOUND = 3.9e-8          # measured at most 3.061e-8 (the same shape: single samples one fp32 ulp away)
# (the 21 fixture cases: 20 bit-identical to the reference-made output, n20 with 1 sample of 69 differing, 1.4e-15 / 3.3e-15)

CASES = R.load_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def case(name):
    return CASES[IDS.index(name)]


def run(c):
    return fa.audio_repitch(c["x"], c["sr"], c["inv"], c["g"], c["quality"])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_against_the_reference_made_output(c):
    y = run(c)
    assert y.shape == c["out"].shape
    rel_rms, rel_max = R.errors(y, c["out"])
    differ = int(np.sum(y.view(np.uint32) != c["out"].view(np.uint32)))
    print("%s: rel_rms=%.3e rel_max=%.3e, %d of %d samples differ" % (c["name"], rel_rms, rel_max, differ, y.size))
    if c["quality"] == R.UNINTERPOLATED:
        assert differ == 0                                                 # copies of input samples
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)
    reached = c["blocks"] * c["g"]
    assert not np.any(y[:, reached:])                                      # what no block reaches stays 0


def test_host_and_device_forms_are_bit_identical():
    dev = torch.device("cuda", 0)
    for name in ("down0p7", "sweep", "u_up1p5", "zero"):
        c = case(name)
        ch, n = c["x"].shape
        y_host = run(c)
        d_x = torch.from_numpy(c["x"]).to(dev)
        d_out = torch.empty((ch, c["out_frames"]), dtype=torch.float32, device=dev)
        d_out.fill_(float("nan"))
        d_ws = torch.empty(fa.audio_repitch_workspace_bytes(n, c["sr"], c["inv"], c["g"], c["quality"]), dtype=torch.uint8, device=dev)
        d_ws.fill_(0xFF)                                                   # no reliance on zeroed workspace
        fa.audio_repitch_dev(d_x, ch, n, c["sr"], c["inv"], c["g"], c["quality"], d_out, d_ws)
        torch.cuda.synchronize()
        y_dev = d_out.cpu().numpy()
        assert np.array_equal(y_host.view(np.uint32), y_dev.view(np.uint32)), name


def test_two_runs_are_bit_identical():
    for name in ("p8_gcd5", "sweep"):
        a, b = run(case(name)), run(case(name))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_channels_are_independent():
    for name in ("down0p7", "p8_gcd5", "u_down0p7"):
        c = case(name)
        y = run(c)
        for k in range(3):
            mono = fa.audio_repitch(c["x"][k:k + 1], c["sr"], c["inv"], c["g"], c["quality"])
            assert np.array_equal(y[k].view(np.uint32), mono[0].view(np.uint32)), (name, k)


@pytest.mark.parametrize("factor,peak_hz", [(1.5, 1500.0), (0.7, 700.0)])
def test_a_sine_moves_to_factor_times_its_frequency(factor, peak_hz):
    sr, n, g = 48000.0, 12000, 48                                          # 0.25 s of 1 kHz
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(F32)[None, :]
    inv = R.invert(np.full(R.factor_count(n, g), factor, F32))
    y = fa.audio_repitch(x, sr, inv, g)
    blocks = len(R.plan(n, sr, inv, g))
    body = y[0, :min(y.shape[1], blocks * g)].astype(np.float64)
    spectrum = np.abs(np.fft.rfft(body * np.hanning(body.size)))
    got_hz = np.argmax(spectrum) * sr / body.size
    print("factor %g: peak at %.1f Hz (bin width %.1f Hz)" % (factor, got_hz, sr / body.size))
    assert abs(got_hz - peak_hz) <= sr / body.size
    # against the smooth fp64 truth: no worse than twice the restatement's own error on the same input (they differ in table rounding only)
    truth = R.smooth_truth(x, sr, factor, y.shape[1])[:, :body.size]
    own_rms, own_max = R.errors(R.repitch(x, sr, inv, g)[:, :body.size], truth)
    rel_rms, rel_max = R.errors(y[:, :body.size], truth)
    print("factor %g: against the smooth truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)" % (factor, rel_rms, rel_max, own_rms, own_max))
    assert rel_rms <= 2 * own_rms and rel_max <= 2 * own_max


def random_case(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 5001))
    ch = int(rng.integers(1, 4))
    g = int(rng.choice([1, 7, 48, 100, 480, 6000])) if n <= 1000 else int(rng.choice([48, 100, 480, 6000]))
    count = R.factor_count(n, g)
    kind = int(rng.integers(0, 4))
    t = np.arange(count) / max(count - 1, 1)
    if kind == 0:
        v = np.full(count, rng.choice([0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 3.0, 0.9, 1.7]))
    elif kind == 1:
        lo, hi = sorted(rng.uniform(0.3, 3.0, 2))
        v = lo + (hi - lo) * t
    elif kind == 2:
        v = 1.0 + 0.6 * np.sin(2 * np.pi * rng.uniform(0.5, 4.0) * t)
    else:
        v = rng.choice([0.5, 1.0, 1.5, 2.0], count)
    quality = R.UNINTERPOLATED if seed % 5 == 4 else R.SINC
    x = (0.5 * rng.standard_normal((ch, n))).astype(F32)
    return x, 48000.0, R.invert(v.astype(F32)), g, quality


@pytest.mark.parametrize("seed", range(20))
def test_random_shapes_against_the_restatement(seed):
    x, sr, inv, g, quality = random_case(seed)
    want = R.repitch(x, sr, inv, g, quality)
    y = fa.audio_repitch(x, sr, inv, g, quality)
    assert y.shape == want.shape
    rel_rms, rel_max = R.errors(y, want)
    print("seed %d: ch=%d n=%d g=%d q=%d -> %d frames  rel_rms=%.3e rel_max=%.3e" % (seed, x.shape[0], x.shape[1], g, quality, y.shape[1], rel_rms, rel_max))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)
