"""Audio::convolve on the MI355X (flan_amd/csrc/conv.hip) against the fp64 truth (tests/convolve_reference.py).
Bounds: DESIGN.md 4.12 lists the measured values they are set from (<= 30 % above)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import convolve_reference as R

pytestmark = pytest.mark.gpu
SR = 48000.0
F32 = np.float32
# against the fp64 truth, normalize off: relative rms error, and max abs error / max |y|
REL_RMS_BOUND = 4.3e-7          # measured at most 3.37e-7 (noise 10 s * noise 10 s)
REL_MAX_BOUND = 9.7e-7          # measured at most 7.50e-7 (tone 10 s * reverb 1 s)


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def signal(kind, ch, n, seed=0):
    rng = np.random.default_rng(seed)
    if kind == "noise":
        return (0.5 * rng.standard_normal((ch, n))).astype(F32)
    if kind == "reverb":                                                   # decaying noise, 60 dB over the length
        return (rng.standard_normal((ch, n)) * np.exp(-6.9 * np.arange(n) / n)).astype(F32)
    if kind == "impulse":
        h = np.zeros((ch, n), F32)
        h[:, min(n - 1, 100)] = 1.0
        return h
    if kind == "silence":
        return np.zeros((ch, n), F32)
    t = np.arange(n) / SR                                                   # tone
    return np.stack([0.4 * np.sin(2 * np.pi * (440.0 + 310.0 * c) * t) + 0.1 * np.sin(2 * np.pi * 3100.0 * t) for c in range(ch)]).astype(F32)


def check_truth(x, h, label):
    y = fa.convolve(x, h, SR, normalize=False)
    assert y.shape == (x.shape[0], x.shape[1] + h.shape[1])
    t = R.truth(x, h)
    rel_rms, rel_max = R.errors(y, t)
    print("%s: P=%d rel_rms=%.3e rel_max=%.3e" % (label, fa.convolve_partition(x.shape[1], h.shape[1]), rel_rms, rel_max))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)
    return y


# (x kind, channels, n, h kind, IR channels, m)
CASES = [
    ("noise", 1, 1, "noise", 1, 1),                     # n = m = 1
    ("noise", 1, 5, "noise", 1, 3000),                  # m > n
    ("noise", 1, 300, "noise", 1, 200),                 # n < P
    ("noise", 1, 10_007, "noise", 1, 513),              # lengths that are not multiples of P
    ("tone", 2, 48_123, "reverb", 1, 4097),             # 2 channels with a mono IR
    ("noise", 1, 20_000, "noise", 2, 777),              # a stereo IR on a mono input: its channel 0 only
    ("noise", 3, 30_001, "reverb", 2, 9000),            # 3 channels with 2 IR channels: 0, 1, 0
    ("noise", 2, 96_000, "impulse", 1, 2000),           # an impulse IR
    ("tone", 1, 480_000, "reverb", 1, 48_000),          # tone 10 s with a 1 s reverb
    ("noise", 1, 480_000, "noise", 1, 480_000),         # 10 s with 10 s (P = 4096, K = 118)
    ("noise", 2, 2_880_000, "reverb", 2, 144_000),      # 60 s stereo with a 3 s stereo reverb
]


@pytest.mark.parametrize("xk,ch,n,hk,irch,m", CASES)
def test_against_fp64_truth(xk, ch, n, hk, irch, m):
    x = signal(xk, ch, n, seed=n)
    h = signal(hk, irch, m, seed=m + 1)
    check_truth(x, h, "%s %dx%d * %s %dx%d" % (xk, ch, n, hk, irch, m))


def test_channel_cycling():
    x = signal("noise", 3, 5000, seed=1)
    h = signal("noise", 2, 700, seed=2)
    y = fa.convolve(x, h, SR, normalize=False)
    # channel 2 uses IR channel 0: the same as convolving channel 2 alone with IR channel 0
    y2 = fa.convolve(x[2:3], h[0:1], SR, normalize=False)
    np.testing.assert_array_equal(y[2], y2[0])
    y1 = fa.convolve(x[1:2], h, SR, normalize=False)                      # a 2-channel IR on a mono input: channel 0 only
    np.testing.assert_array_equal(y1[0], fa.convolve(x[1:2], h[0:1], SR, normalize=False)[0])


def test_partition_invariance():
    x = signal("noise", 2, 30_000, seed=5)
    h = signal("reverb", 1, 4096, seed=6)
    t = R.truth(x, h)
    outs = {}
    for P in (128, 512, 1024, 4096):                                      # K = 32, 8, 4, 1
        with fa.convolve_partition_forced(P):
            outs[P] = fa.convolve(x, h, SR, normalize=False)
        rel_rms, rel_max = R.errors(outs[P], t)
        print("P=%d K=%d rel_rms=%.3e rel_max=%.3e" % (P, -(-4096 // P), rel_rms, rel_max))
        assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND
    scale = np.max(np.abs(t))
    for P in (128, 512, 1024):
        assert np.max(np.abs(outs[P].astype(np.float64) - outs[4096])) <= 2 * REL_MAX_BOUND * scale


def test_host_and_device_forms_are_bit_identical():
    dev = torch.device("cuda", 0)
    for normalize in (False, True):
        x = signal("tone", 2, 100_000, seed=7)
        h = signal("reverb", 1, 20_000, seed=8)
        ch, n = x.shape
        irch, m = h.shape
        y_host = fa.convolve(x, h, SR, normalize=normalize)
        d_x = torch.from_numpy(x).to(dev)
        d_h = torch.from_numpy(h).to(dev)
        d_out = torch.empty((ch, n + m), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.convolve_workspace_bytes(ch, n, irch, m), dtype=torch.uint8, device=dev)
        d_ws.fill_(0xFF)                                                   # no reliance on zeroed workspace
        fa.convolve_dev(d_x, ch, n, d_h, irch, m, SR, normalize, d_out, d_ws)
        torch.cuda.synchronize()
        y_dev = d_out.cpu().numpy()
        assert np.array_equal(y_host.view(np.uint32), y_dev.view(np.uint32))


def test_two_runs_are_bit_identical():
    x = signal("noise", 2, 200_000, seed=9)
    h = signal("reverb", 2, 50_000, seed=10)
    a = fa.convolve(x, h, SR, normalize=True)
    b = fa.convolve(x, h, SR, normalize=True)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_silence():
    x = signal("silence", 2, 10_000)
    h = signal("reverb", 1, 3000, seed=11)
    y = fa.convolve(x, h, SR, normalize=False)
    assert np.all(y == 0.0)
    yn = fa.convolve(x, h, SR, normalize=True)
    assert np.all(np.isnan(yn))                                            # 0 * (1.0f / 0): the reference's NaN
    np.testing.assert_array_equal(np.isnan(yn), np.isnan(R.restatement(x, h, SR, normalize=True)))


@pytest.mark.parametrize("n,m", [(1, 1), (1000, 10), (48_000, 4800), (300_001, 30_000)])
def test_normalize_is_the_reference_gain_to_the_bit(n, m):
    x = signal("tone", 2, n, seed=12)
    h = signal("reverb", 1, m, seed=13)
    y0 = fa.convolve(x, h, SR, normalize=False)
    y1 = fa.convolve(x, h, SR, normalize=True)
    expect = R.normalized(y0, SR)                                          # out * ( 1.0f / max over [0, end) )
    nan = np.isnan(expect)                                                 # (a 0 max: NaN, whose bits the CPU and the GPU spell differently)
    np.testing.assert_array_equal(np.isnan(y1), nan)
    assert np.array_equal(y1[~nan].view(np.uint32), expect[~nan].view(np.uint32))
