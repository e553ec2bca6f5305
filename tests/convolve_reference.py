"""Audio::convolve (Audio/AudioCombination.cpp:299-352) restated in numpy, and the fp64 truth the GPU is measured against.

restatement(): the reference's algorithm in fp32 -- one real transform of size D = 2 pow2( max( n, m ) ) per channel (FFTHelper.cpp:11-14),
both inputs pre-scaled by 1 / sqrt( D ) (a double quotient stored as float), spectra multiplied, an unnormalised c2r, the first n + m
samples kept, IR channels used cyclically; with normalize, out * ( 1.0f / max ) over the frame range of
AudioBuffer::get_max_sample_magnitude() (AudioBuffer.cpp:416-430).  numpy 2.x transforms float32 in float32 (pocketfft), so this is an
fp32 FFT like the reference's FFTW plan, though not FFTW's rounding.
truth(): the exact linear convolution in fp64, n + m frames (the last one exactly 0)."""
import numpy as np

F32 = np.float32


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
