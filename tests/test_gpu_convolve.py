"""Audio::convolve on the MI355X (flan_amd/csrc/conv.hip) against the fp64 truth (tests/convolve_reference.py).
Global bounds: DESIGN.md 4.12 lists the measured values they are set from (<= 30 % above).
The local criterion (check_local): per (channel, partition of P frames) the error is measured in units of s[c][j], the Cauchy-Schwarz bound of
that partition's samples; where s is 0 the device gives exactly 0, and elsewhere its worst figure is at most R.LOCAL_FACTOR times the worst
figure of the numpy fp32 model of the same algorithm on the same case.  The two global figures cannot see a fault in a quiet partition or
a quiet channel (tests/test_convolve_reference.py plants three and shows it); this one can."""
import contextlib

import numpy as np
import pytest
import torch

import flan_amd as fa
import convolve_reference as R
from convolve_reference import REL_RMS_BOUND, REL_MAX_BOUND    # against the fp64 truth, normalize off: 4.3e-7 rms, 9.7e-7 max / max |y|

pytestmark = pytest.mark.gpu
SR = 48000.0
F32 = np.float32


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


# ---------------------------------------------------------------------------------------------------------------
# The local criterion: every partition against the truth, in units of its own scale
# ---------------------------------------------------------------------------------------------------------------

def forced(P):
    """the library's own choice for P = None"""
    return fa.convolve_partition_forced(P) if P else contextlib.nullcontext()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_local(x, h, P, label, force=True):
    """run at partition P (forced, or the library's own choice, which must then be P) and hold the output to the local criterion"""
    if not force:
        assert fa.convolve_partition(x.shape[1], h.shape[1]) == P
    with forced(P if force else None):
        y = fa.convolve(x, h, SR, normalize=False)
    t = R.local_truth(x, h)
    dev, model, stray = R.local_figures(y, x, h, P, t)
    print("%s: P=%d K=%d device %.3f model %.3f (2^-24 s) ratio %.2f stray %d; global rel_rms=%.3e rel_max=%.3e" % (
        (label, P, -(-h.shape[1] // P), dev / R.ULP, model / R.ULP, dev / model if model else np.inf, stray) + R.errors(y, t)))
    assert stray == 0                                                      # exactly 0 wherever every term of the sum is
    assert dev <= R.LOCAL_FACTOR * model, (dev / R.ULP, model / R.ULP)
    return y, model


@pytest.mark.parametrize("K", R.K_TABLE)
def test_local_K_table(K):
    # K around the 16-slot ring and the 32 of the library's rule; J = 19 + K or 20 + K: several tiles, a ragged last one, Jx = 21 < J
    x, h = R.k_table_case(K)
    check_local(x, h, 128, "K table %d" % K)


@pytest.mark.parametrize("P", [128, 256, 512, 1024, 2048, 4096])
def test_local_P_table(P):
    x, h = R.quiet_pair(2, 5 * P + 3, 1, 3 * P - 5, seed=P)
    check_local(x, h, P, "P table %d" % P)


@pytest.mark.parametrize("m,P,K", [(16384, 512, 32), (16385, 1024, 17), (131072, 4096, 32), (131073, 4096, 33)])
def test_local_at_the_edges_of_the_partition_rule(m, P, K):
    assert -(-m // P) == K
    x, h = R.quiet_pair(1, 2 * P + 1, 1, m, seed=m)
    check_local(x, h, P, "own choice m=%d" % m, force=False)


@pytest.mark.parametrize("xk,ch,n,hk,irch,m", CASES[:5])
def test_local_on_the_small_cases(xk, ch, n, hk, irch, m):
    x = signal(xk, ch, n, seed=n)
    h = signal(hk, irch, m, seed=m + 1)
    check_local(x, h, fa.convolve_partition(n, m), "%s %dx%d * %s %dx%d" % (xk, ch, n, hk, irch, m), force=False)


@pytest.mark.parametrize("P,force", [(128, True), (512, False)])
def test_local_impulse_grid(P, force):
    """single ( i, j - i ) terms walked through every ring slot and tile edge with nothing else in the sum"""
    x, h, a, b = R.impulse_grid(128)
    K, J = R.partitions(x.shape[1], h.shape[1], P)
    assert (K, J) == ((34, 70) if P == 128 else (9, 18))
    y, model = check_local(x, h, P, "impulse grid", force=force)
    s = R.partition_scale(x, h, P)
    if P == 128:
        assert np.mean(s == 0) >= 0.97                                     # (all of which check_local found exactly 0)
    c = np.arange(100)
    product = x[c, a].astype(np.float64) * h[c % 10, b]
    assert np.all(np.abs(y[c, a + b] - product) <= R.LOCAL_FACTOR * model * s[c, (a + b) // P])
    assert np.all(np.abs(y[c, a + b]) >= 0.99 * np.abs(product))


@pytest.mark.parametrize("P", [128, 512])
def test_containment_bit_for_bit(P):
    K = 5
    n, m, q, r = 20 * P + 9, K * P - 3, 7 * P + 5, 2 * P + 1
    x, h = R.quiet_pair(3, n, 2, m, seed=20 + P)
    other_x, other_h = R.quiet_pair(3, n, 2, m, seed=21 + P)
    with forced(P):
        y = fa.convolve(x, h, SR, normalize=False)
        # causality in the input: what comes from frame q on reaches no partition before q's
        x2 = x.copy()
        x2[:, q:] = other_x[:, q:]
        y2 = fa.convolve(x2, h, SR, normalize=False)
        assert np.array_equal(bits(y2[:, : q // P * P]), bits(y[:, : q // P * P]))
        assert all(not np.array_equal(y2[c, q : q + m], y[c, q : q + m]) for c in range(3))
        # and in the IR
        h2 = h.copy()
        h2[:, r:] = other_h[:, r:]
        y3 = fa.convolve(x, h2, SR, normalize=False)
        assert np.array_equal(bits(y3[:, : r // P * P]), bits(y[:, : r // P * P]))
        assert all(not np.array_equal(y3[c, r:], y[c, r:]) for c in range(3))
        # a NaN stays in its channel and in the partitions whose sums hold one of the two spectra it is in
        xn = x.copy()
        xn[1, q] = np.nan
        yn = fa.convolve(xn, h, SR, normalize=False)
        yn_norm = fa.convolve(xn, h, SR, normalize=True)
    lo, hi = q // P * P, min((q // P + K + 1) * P, n + m)
    assert np.array_equal(bits(yn[[0, 2]]), bits(y[[0, 2]]))
    assert np.array_equal(bits(yn[1, :lo]), bits(y[1, :lo])) and np.array_equal(bits(yn[1, hi:]), bits(y[1, hi:]))
    assert not np.any(np.isfinite(yn[1, q : q + m]))
    model = R.partitioned(xn, h, P)                                        # the same window on the CPU
    assert np.all(np.isfinite(model[1, :lo])) and np.all(np.isfinite(model[1, hi:])) and not np.any(np.isfinite(model[1, lo:hi]))
    # normalize: the kernel's fmaxf and the reference's `>` both skip the NaN
    finite = np.isfinite(yn)
    expect = R.normalized_skipping_nan(yn, SR)
    assert np.isfinite(R.max_magnitude_skipping_nan(yn, SR)) and R.max_magnitude_skipping_nan(yn, SR) > 0
    np.testing.assert_array_equal(np.isfinite(yn_norm), finite)
    assert np.array_equal(bits(yn_norm[finite]), bits(expect[finite]))


def test_a_channel_alone_and_among_many():
    P, K = 128, 17
    x, h = R.quiet_pair(5, 19 * P + 3, 3, K * P - 5, seed=30)
    with forced(P):
        y = fa.convolve(x, h, SR, normalize=False)
        for c in range(5):
            alone = fa.convolve(x[c : c + 1], h[c % 3 : c % 3 + 1], SR, normalize=False)
            assert np.array_equal(bits(alone[0]), bits(y[c])), c
        # reversed: channel c' = 4 - c must meet the IR channel it met before, so the IR is laid out for c' % 3
        hr = np.stack([h[(4 - k) % 3] for k in range(3)])
        yr = fa.convolve(x[::-1], hr, SR, normalize=False)
    assert np.array_equal(bits(yr), bits(y[::-1]))


# 5 channels x 28 partitions = 140 inverse blocks, block b = c J + j to word b mod 64 of the 64 maxima
NORM_CH, NORM_P, NORM_N, NORM_M = 5, 128, 26 * 128 + 10, 128 + 64


@pytest.mark.parametrize("block", [0, 63, 64, 127, 139])
def test_normalize_maximum_in_a_chosen_slot(block):
    P, n, m = NORM_P, NORM_N, NORM_M
    K, J = R.partitions(n, m, P)
    assert (K, J) == (2, 28) and NORM_CH * J - 1 == 139
    c, j = divmod(block, J)
    tap = 0 if j < J - 1 else m - 20                                       # the last partition lies past the input: reach it through the IR
    rng = np.random.default_rng(block)
    h = (1e-3 * rng.standard_normal((1, m))).astype(F32)
    h[0, tap] = 3.0
    x = np.zeros((NORM_CH, n), F32)
    start = j * P + 5 - tap
    x[c, start : start + 8] = (0.5 + rng.random(8)).astype(F32)            # one loud burst in a silent input
    with forced(P):
        y0 = fa.convolve(x, h, SR, normalize=False)
        y1 = fa.convolve(x, h, SR, normalize=True)
    end = R.norm_end(n + m, SR)
    pc, pf = np.unravel_index(np.argmax(np.abs(y0[:, :end])), (NORM_CH, end))
    assert (pc, pf // P) == (c, j)                                         # the peak is in the inverse block this case names
    assert np.array_equal(bits(y1), bits(R.normalized(y0, SR)))


def test_normalize_maximum_at_the_last_frame_of_the_range():
    P, n, m = NORM_P, NORM_N, NORM_M
    x = np.zeros((NORM_CH, n), F32)
    h = np.zeros((1, m), F32)
    x[3, n - 1] = -0.7
    h[0, m - 1] = 0.3
    with forced(P):
        y0 = fa.convolve(x, h, SR, normalize=False)
        y1 = fa.convolve(x, h, SR, normalize=True)
    assert R.norm_end(n + m, SR) == n + m - 1                              # frames [0, n + m - 1): n + m - 2 is the last one in the range
    only = np.zeros_like(y0, dtype=bool)
    only[3, n + m - 2] = True
    assert np.all(np.abs(y0[~only]) < 1e-7) and abs(y0[3, n + m - 2] + 0.21) < 1e-6
    assert np.array_equal(bits(y1), bits(R.normalized(y0, SR)))
    assert abs(y1[3, n + m - 2] + 1.0) < 1e-6 and np.all(np.abs(y1[~only]) < 1e-6)    # a maximum that missed the frame would be round-off or 0


@pytest.mark.parametrize("P", [128, None])
@pytest.mark.parametrize("normalize", [False, True])
def test_dev_form_stays_inside_out_and_workspace(P, normalize):
    GUARD = 4096
    dev = torch.device("cuda", 0)
    ch, n, irch, m = 3, 19 * 128 + 4, 2, 17 * 128 - 5
    assert (n + m) % 2 == 1
    x, h = R.quiet_pair(ch, n, irch, m, seed=40)
    with forced(P):
        y_host = fa.convolve(x, h, SR, normalize=normalize)
        out_bytes = 4 * ch * (n + m)
        ws_bytes = fa.convolve_workspace_bytes(ch, n, irch, m)
        assert ws_bytes > 0
        d_x = torch.from_numpy(x).to(dev)
        d_h = torch.from_numpy(h).to(dev)
        big_out = torch.full((out_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        big_ws = torch.full((ws_bytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        d_out = big_out[GUARD : GUARD + out_bytes]
        d_ws = big_ws[GUARD : GUARD + ws_bytes]
        fa.convolve_dev(d_x, ch, n, d_h, irch, m, SR, normalize, d_out, d_ws)
        torch.cuda.synchronize()
    for big, size in ((big_out, out_bytes), (big_ws, ws_bytes)):
        host = big.cpu().numpy()
        assert np.all(host[:GUARD] == 0xA5) and np.all(host[GUARD + size :] == 0xA5)
    assert np.array_equal(d_x.cpu().numpy(), x) and np.array_equal(d_h.cpu().numpy(), h)
    y_dev = big_out.cpu().numpy()[GUARD : GUARD + out_bytes].view(F32).reshape(ch, n + m)
    assert np.array_equal(bits(y_dev), bits(y_host))
