"""Audio::convolve (Audio/AudioCombination.cpp:299-352) restated in numpy, and the fp64 truth the GPU is measured against.

restatement(): the reference's algorithm in fp32 -- one real transform of size D = 2 pow2( max( n, m ) ) per channel (FFTHelper.cpp:11-14),
both inputs pre-scaled by 1 / sqrt( D ) (a double quotient stored as float), spectra multiplied, an unnormalised c2r, the first n + m
samples kept, IR channels used cyclically; with normalize, out * ( 1.0f / max ) over the frame range of
AudioBuffer::get_max_sample_magnitude() (AudioBuffer.cpp:416-430).  numpy 2.x transforms float32 in float32 (pocketfft), so this is an
fp32 FFT like the reference's FFTW plan, though not FFTW's rounding.
truth(): the exact linear convolution in fp64, n + m frames (the last one exactly 0).
partitioned(): the GPU's own algorithm (uniformly partitioned overlap-save, conv.hip) in fp32 or fp64; partition_scale(), local_errors(),
local_truth() and local_figures(): the error of an output per (channel, partition) in units of that partition's own scale, which a fault in
a quiet partition or a quiet channel cannot hide from."""
import numpy as np

F32 = np.float32
# The global bounds of tests/test_gpu_convolve.py against the fp64 truth, normalize off: relative rms error, and max abs error / max |y|.
# (Here so that the device-free tests can show what these two numbers let through.)
REL_RMS_BOUND = 4.3e-7          # measured at most 3.37e-7 (noise 10 s * noise 10 s)
REL_MAX_BOUND = 9.7e-7          # measured at most 7.50e-7 (tone 10 s * reverb 1 s)


def pow2_container(n):
    """power_of_2_container( n ) = 2 ^ ceil( log2( n ) )"""
    return 1 << int(np.ceil(np.log2(n))) if n > 1 else 1


def norm_end(num_frames, sample_rate):
    """get_max_sample_magnitude() with default arguments scans frames [0, end): end = clamp( Frame( time_to_frame( get_length() ) ), 0, N-1 )
    with get_length() = float( N ) / sr and time_to_frame( t ) = t * sr, both in fp32"""
    length = F32(num_frames) / F32(sample_rate)
    f = F32(length * F32(sample_rate))
    return int(min(max(int(f), 0), num_frames - 1))


def max_magnitude(out, sample_rate):
    """AudioBuffer::get_max_sample_magnitude() of an [ch][N] float32 buffer, default arguments"""
    end = norm_end(out.shape[1], sample_rate)
    return F32(np.max(np.abs(out[:, :end]))) if end > 0 else F32(0)


def normalized(out, sample_rate):
    """out.modify_volume_in_place( 1.0f / out.get_max_sample_magnitude() ): an fp32 reciprocal, then an fp32 product (inf for a 0 max)"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gain = F32(1) / max_magnitude(out, sample_rate)
        return (out * gain).astype(F32)


def restatement(x, h, sample_rate, normalize=True):
    x = np.asarray(x, F32)
    h = np.asarray(h, F32)
    ch, n = x.shape
    irch, m = h.shape
    D = 2 * pow2_container(max(n, m))
    s = np.sqrt(float(D))
    out = np.empty((ch, n + m), F32)
    for c in range(ch):
        a = np.zeros(D, F32)
        a[:n] = (x[c].astype(np.float64) / s).astype(F32)
        b = np.zeros(D, F32)
        b[:m] = (h[c % irch].astype(np.float64) / s).astype(F32)
        A = np.fft.rfft(a)
        B = np.fft.rfft(b)
        y = np.fft.irfft(A * B, n=D, norm="forward")
        out[c] = y[: n + m].astype(F32)
    return normalized(out, sample_rate) if normalize else out


def truth(x, h):
    """exact fp64 linear convolution, n + m frames: direct sums for small shapes, an fp64 FFT for large ones"""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    ch, n = x.shape
    irch, m = h.shape
    out = np.zeros((ch, n + m), np.float64)
    for c in range(ch):
        hc = h[c % irch]
        if n * m <= 4_000_000:
            out[c, : n + m - 1] = np.convolve(x[c], hc)
        else:
            L = 1 << int(np.ceil(np.log2(n + m)))
            out[c, : n + m - 1] = np.fft.irfft(np.fft.rfft(x[c], L) * np.fft.rfft(hc, L), L)[: n + m - 1]
    return out


def errors(y, t):
    """(relative rms, max abs error / max |t|) of y against the truth t"""
    y = np.asarray(y, np.float64)
    scale = np.max(np.abs(t))
    rel_rms = np.sqrt(np.sum((y - t) ** 2) / np.sum(t ** 2))
    return float(rel_rms), float(np.max(np.abs(y - t)) / scale)


# ---------------------------------------------------------------------------------------------------------------
# The kernel's own algorithm (flan_amd/csrc/conv.hip) in numpy, and the local metric the device is held to
# ---------------------------------------------------------------------------------------------------------------

def partitions(n, m, P):
    """(K, J): IR partitions ceil( m / P ) and output partitions ceil( ( n + m ) / P )"""
    return -(-m // P), -(-(n + m) // P)


def _blocks(v, P, count):
    """v zero-padded and cut into `count` blocks of P: [count][P]"""
    out = np.zeros(count * P, v.dtype)
    out[: v.size] = v[: count * P]
    return out.reshape(count, P)


def partitioned(x, h, P, dtype=np.float32, drop=None):
    """Uniformly partitioned overlap-save as conv.hip runs it: H_i = rfft( h[iP, (i+1)P) zero-padded to 2P ), X_j = rfft( x[(j-1)P, (j+1)P) )
    with zeros outside the input, Y_j = sum of X_{j-i} H_i for i = 0 ... min( j, K-1 ) in that order in complex64 (complex128 for
    dtype=float64), the last P samples of irfft( Y_j ) kept and cropped to n + m; IR channels used cyclically.  drop( i, j ) true skips
    that term (the tests plant defects with it).  numpy 2.x transforms float32 in float32, so dtype=float32 is an fp32 pipeline like
    the kernel's, though not with its roundings."""
    x = np.asarray(x, dtype)
    h = np.asarray(h, dtype)
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    ch, n = x.shape
    irch, m = h.shape
    K, J = partitions(n, m, P)
    spectra = {}
    out = np.empty((ch, J * P), dtype)
    for c in range(ch):
        k = c % irch
        if k not in spectra:
            hb = np.zeros((K, 2 * P), dtype)
            hb[:, :P] = _blocks(h[k], P, K)
            spectra[k] = np.fft.rfft(hb, axis=1).astype(ctype)
        H = spectra[k]
        xb = _blocks(x[c], P, J + 1)                                       # block j + 1 of xw is x[jP, (j+1)P)
        xw = np.zeros((J, 2 * P), dtype)
        xw[1:, :P] = xb[: J - 1]
        xw[:, P:] = xb[:J]
        X = np.fft.rfft(xw, axis=1).astype(ctype)
        Y = np.zeros((J, P + 1), ctype)
        for i in range(min(K, J)):
            term = X[: J - i] * H[i]                                       # the i-th term of Y_j, j = i ... J - 1
            if drop is not None:
                keep = np.array([not drop(i, j) for j in range(i, J)])
                term = term[keep]
                Y[i:][keep] += term
            else:
                Y[i:] += term
        y = np.fft.irfft(Y, n=2 * P, axis=1).astype(dtype)
        out[c] = y[:, P:].reshape(-1)
    return np.ascontiguousarray(out[:, : n + m])


def partition_scale(x, h, P):
    """s[c][j] = sum over i <= min( j, K-1 ) of || x[(j-i-1)P, (j-i+1)P) ||_2 || h_i ||_2 in fp64.  By Cauchy-Schwarz every true output
    sample of partition j is at most s[c][j] in magnitude (each term's circular convolution is), and an fp32 FFT pair plus accumulation
    rounds in proportion to it.  Exactly 0 where every term of the partition is 0."""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    ch, n = x.shape
    irch, m = h.shape
    K, J = partitions(n, m, P)
    s = np.zeros((ch, J))
    hn = [np.sqrt(np.sum(_blocks(h[k], P, K) ** 2, axis=1)) for k in range(irch)]
    for c in range(ch):
        e = np.sum(_blocks(x[c], P, J + 1) ** 2, axis=1)                   # energy of x[jP, (j+1)P)
        xn = np.sqrt(e[:J] + np.concatenate(([0.0], e[: J - 1])))           # || x[(j-1)P, (j+1)P) ||
        s[c] = np.convolve(xn, hn[c % irch])[:J]                           # direct sums of non-negative terms: 0 stays exactly 0
    return s


def local_errors(y, t, s, P):
    """max | y - t | / s per (channel, partition of P frames), 0 where s == 0"""
    y = np.asarray(y, np.float64)
    ch, N = t.shape
    J = s.shape[1]
    d = np.zeros((ch, J * P))
    d[:, :N] = np.abs(y - t)
    worst = d.reshape(ch, J, P).max(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, worst / s, 0.0)


def local_truth(x, h):
    """fp64 linear convolution, n + m frames, whose error stays local: np.convolve's direct sums up to n m = 4e6, else the partitioned
    algorithm in fp64 at P = 4096.  (truth()'s one big FFT errs by about 1e-16 of the GLOBAL peak, more than a quiet partition holds.)"""
    x = np.asarray(x, np.float64)
    h = np.asarray(h, np.float64)
    ch, n = x.shape
    irch, m = h.shape
    if n * m > 4_000_000:
        return partitioned(x, h, 4096, dtype=np.float64)
    out = np.zeros((ch, n + m), np.float64)
    for c in range(ch):
        out[c, : n + m - 1] = np.convolve(x[c], h[c % irch])
    return out


def max_magnitude_skipping_nan(out, sample_rate):
    """get_max_sample_magnitude() as its loop runs on a buffer that holds NaN: `if( abs( s ) > max ) max = abs( s )` is false for a NaN,
    so the maximum is over the other samples of the range (np.max would hand the NaN on)"""
    end = norm_end(out.shape[1], sample_rate)
    return F32(np.fmax.reduce(np.abs(out[:, :end]), axis=None, initial=F32(0))) if end > 0 else F32(0)


def normalized_skipping_nan(out, sample_rate):
    """normalized() with the maximum that skips NaN"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        gain = F32(1) / max_magnitude_skipping_nan(out, sample_rate)
        return (out * gain).astype(F32)


# The local criterion: where s == 0 an output is exactly 0, elsewhere its worst local error is at most LOCAL_FACTOR times
# the worst local error of partitioned( fp32 ) on the same case.  4 is the factor the multinotch truth criterion allows between a device
# and its fp32 restatement.  Measured on the MI355X: 1.00 - 2.16 times the model over tests/test_gpu_convolve.py's cases, so
# 4 stands; the smallest planted defect sits thousands of times above it.
LOCAL_FACTOR = 4.0
ULP = 2.0 ** -24


def local_figures(y, x, h, P, t=None):
    """(worst local error of y, worst local error of the fp32 model, number of non-zero samples of y in partitions with s == 0); errors in
    units of s[c][j], against t = local_truth( x, h )"""
    t = local_truth(x, h) if t is None else t
    s = partition_scale(x, h, P)
    silent = np.repeat(s == 0, P, axis=1)[:, : t.shape[1]]
    stray = int(np.count_nonzero(np.asarray(y)[silent]))
    return float(local_errors(y, t, s, P).max()), float(local_errors(partitioned(x, h, P), t, s, P).max()), stray


def quiet_pair(ch, n, irch, m, seed):
    """the signals of the local tests: noise whose channel 1 is 1e-4 of channel 0, and an IR of noise decaying 140 dB over its length"""
    rng = np.random.default_rng(seed)
    x = (0.5 * rng.standard_normal((ch, n))).astype(F32)
    if ch > 1:
        x[1] *= F32(1e-4)
    h = (rng.standard_normal((irch, m)) * np.exp(-16.1 * np.arange(m) / m)).astype(F32)
    return x, h


def k_table_case(K, P=128):
    """2 ch x ( 19 P + 3 ) with 2 IR channels of K P - 5: J spans several 16-tiles with a ragged last one, and Jx < J"""
    return quiet_pair(2, 19 * P + 3, 2, K * P - 5, seed=1000 + K)


K_TABLE = (1, 2, 15, 16, 17, 31, 32, 33, 34, 48, 49)


def impulse_grid(P=128):
    """100 input channels x 10 IR channels of single samples: IR channel k holds 0.37 10^-k at b_k, input channel 10 ia + k holds -1.7 at
    a_ia, so that channel cycling pairs every a with every b.  Returns x, h, a (per input channel), b (per input channel)."""
    m, n = 34 * P - 5, 35 * P + 7
    bs = [0, P - 1, P, 15 * P + 3, 16 * P - 1, 16 * P, 31 * P, 32 * P, 33 * P, m - 1]
    as_ = [0, 1, P - 1, P, P + 1, 15 * P, 16 * P - 1, 16 * P, 17 * P, n - 1]
    h = np.zeros((10, m), F32)
    for k, b in enumerate(bs):
        h[k, b] = F32(0.37 * 10.0 ** -k)
    x = np.zeros((100, n), F32)
    for ia, a in enumerate(as_):
        for k in range(10):
            x[10 * ia + k, a] = F32(-1.7)
    return x, h, np.repeat(as_, 10), np.tile(bs, 10)
