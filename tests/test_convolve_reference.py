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


# ---------------------------------------------------------------------------------------------------------------
# partitioned(): the kernel's algorithm, its fp64 form as a truth, and the local metric
# ---------------------------------------------------------------------------------------------------------------

# (P, K, n): K below, at and above 16 and 32, ragged n and m = K P - 5
PARTITIONED_SHAPES = [(128, 1, 77), (128, 15, 1000), (128, 16, 2435), (128, 17, 300), (128, 31, 1), (128, 32, 2435), (128, 33, 129),
                      (128, 40, 2500), (512, 1, 1500), (512, 3, 2563), (512, 17, 513)]


@pytest.mark.parametrize("P,K,n", PARTITIONED_SHAPES)
def test_partitioned_fp64_is_np_convolve_partition_by_partition(P, K, n):
    x, h = R.quiet_pair(2, n, 2, K * P - 5, seed=P + K)
    assert R.partitions(n, K * P - 5, P)[0] == K
    y = R.partitioned(x, h, P, dtype=np.float64)
    assert y.dtype == np.float64 and y.shape == (2, n + K * P - 5)
    t = _direct(x, h)
    e = R.local_errors(y, t, R.partition_scale(x, h, P), P)
    assert e.max() <= 1e-12, e.max()


def test_partition_scale_bounds_every_true_sample_and_is_zero_where_the_output_is():
    x, h = R.quiet_pair(2, 1500, 2, 17 * 128 - 5, seed=4)
    x[:, 300:1100] = 0                                                   # a silent stretch longer than what is left of the IR
    h[:, 128:] = 0
    t = _direct(x, h)
    s = R.partition_scale(x, h, 128)
    assert R.local_errors(np.zeros_like(t), t, s, 128).max() <= 1.0      # |t| <= s
    assert np.count_nonzero(s == 0) > 0
    assert not np.any(t[np.repeat(s == 0, 128, axis=1)[:, : t.shape[1]]])
    np.testing.assert_array_equal(R.local_truth(x, h), t)


def test_local_truth_above_the_direct_limit_stays_local():
    x, h = R.quiet_pair(2, 5000, 1, 4096, seed=5)                        # n m above the direct-sum limit
    x[:, 2000:] = 0
    t = R.local_truth(x, h)
    d = _direct(x, h)
    assert R.local_errors(t, d, R.partition_scale(x, h, 4096), 4096).max() <= 1e-12
    assert not np.any(t[:, 3 * 4096:])                                   # what must be 0 is 0, which truth()'s one big FFT does not give


def test_model_distance_on_the_K_table():
    worst = 0.0
    for K in R.K_TABLE:
        x, h = R.k_table_case(K)
        _, model, _ = R.local_figures(np.zeros((2, x.shape[1] + h.shape[1])), x, h, 128)
        print("K=%d model %.3f ulp" % (K, model / R.ULP))
        worst = max(worst, model)
    assert worst < 1.0 * R.ULP, worst / R.ULP                            # measured 0.37 - 0.53


def test_model_distance_on_the_impulse_grid():
    x, h, a, b = R.impulse_grid(128)
    y = R.partitioned(x, h, 128)
    dev, model, stray = R.local_figures(y, x, h, 128)
    print("impulse grid: model %.3f ulp" % (model / R.ULP))
    assert dev == model and model < 4.0 * R.ULP, model / R.ULP           # measured 2.06
    assert stray == 0                                                    # the fp32 model too is exactly 0 where every term is


def test_model_contains_a_nan_like_the_kernel():
    P, K = 128, 5
    x, h = R.quiet_pair(3, 20 * P + 9, 1, K * P - 3, seed=6)
    y0 = R.partitioned(x, h, P)
    x[1, 7 * P + 5] = np.nan                                             # frame 901
    y = R.partitioned(x, h, P)
    bad = ~np.isfinite(y)
    assert not bad[0].any() and not bad[2].any()
    assert bad[1, 896:1664].all() and not bad[1, :896].any() and not bad[1, 1664:].any()
    assert np.array_equal(y[~bad].view(np.uint32), y0[~bad].view(np.uint32))
    # the NaN-skipping maximum sees the finite samples only
    assert R.max_magnitude_skipping_nan(y, SR) == np.max(np.abs(y[~bad & (np.arange(y.shape[1]) < R.norm_end(y.shape[1], SR))]))
    assert np.isnan(R.max_magnitude(y, SR))


# the three defects of DESIGN.md 4.12, each a term of the delay line that is never added: (n, m, drop)
DEFECTS = [
    pytest.param(3000, 4096, lambda i, j: i == 31, id="last IR partition of 32 dropped"),
    pytest.param(3000, 4096, lambda i, j: i == 31 and j % 16 == 15, id="the same in the last slot of a 16-tile only"),
    pytest.param(2500, 5000, lambda i, j: i == 39, id="last IR partition of 40 dropped"),
]


@pytest.mark.parametrize("n,m,drop", DEFECTS)
def test_planted_defects_pass_the_global_bounds_and_break_the_local_criterion(n, m, drop):
    """Why the local criterion exists: a late, quiet IR partition that is never added moves the two global figures of
    test_gpu_convolve.py by less than their bounds allow, and the local figure by thousands of times its allowance."""
    x, h = R.quiet_pair(2, n, 1, m, seed=n)
    bad = R.partitioned(x, h, 128, drop=drop)
    rel_rms, rel_max = R.errors(bad, R.truth(x, h))
    assert rel_rms <= R.REL_RMS_BOUND and rel_max <= R.REL_MAX_BOUND, (rel_rms, rel_max)
    fig, model, _ = R.local_figures(bad, x, h, 128)
    print("defect %.3g ulp, model %.3f ulp: %.3g times the allowance" % (fig / R.ULP, model / R.ULP, fig / (R.LOCAL_FACTOR * model)))
    assert model < 1.0 * R.ULP
    assert fig > 100 * R.LOCAL_FACTOR * model


def test_silence_normalizes_to_nan():
    x = np.zeros((1, 50), np.float32)
    h = np.ones((1, 5), np.float32)
    assert np.all(R.restatement(x, h, SR, normalize=False) == 0)
    assert np.all(np.isnan(R.restatement(x, h, SR, normalize=True)))
