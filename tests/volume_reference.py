"""NumPy restatement of what flan_amd/csrc/volume.hip and the C++ methods over it compute (Audio/AudioVolume.cpp:15-30, 69-188, 280-321,
Function.cpp:11-39, Audio/AudioInformation.cpp:121-136, 320-363, Audio/AudioSynthesis.cpp:25-89).  For every numeric path there are two
functions: an fp64 TRUTH (the inputs are the fp32 values, every operation after that is fp64) and an fp32 RESTATEMENT (np.float32
operations in the reference's order).  The reference's constant pi2 = acos( -1.0f ) * 2.0f is an fp32 INPUT of both: the truth measures
roundings, not the constant.  Where the reference picks a curve entry by fp32 arithmetic (Frame( t * sr )) both use that fp32 index: it
selects, it does not round.

  ring_modulate, fade_plan, fade_tables, fade_frames, invert_phase          exact paths
  waveform( kind, t ), waveform_truth( kind, t )
  moisture( ... ), moisture_truth( ... ), curve_index( ... )
  phases_truth( freq, M ), phases_fp32( freq, M ), circular_distance( a, b )
  energy_truth( x )
  adsr( t, ... )
  white_noise_draw( seed, count )
  hann_window( width_frames ), envelope_function( ys, sr, t )
  synthesize_waveform_frames( length, sr, oversample )
"""
import math

import numpy as np

from temporal_reference import MT19937

F32 = np.float32
PI = F32(np.arccos(F32(-1.0)))                  # std::acos( -1.0f )
PI2 = F32(PI * F32(2.0))                        # defines.h:45
SINE, SQUARE, SAW, TRIANGLE = 0, 1, 2, 3


# ---- exact paths -------------------------------------------------------------------------------------------------------------------------
def ring_modulate(x, other):
    """AudioVolume.cpp:26"""
    x, other = np.atleast_2d(x).astype(F32), np.atleast_2d(other).astype(F32)
    ch, n = x.shape
    c = np.arange(ch) % other.shape[0]
    f = np.arange(n) % other.shape[1]
    return (x * other[c][:, f]).astype(F32)


def fade_plan(n, start, end):
    """AudioVolume.cpp:111-118, in fp32; the sum of the two lengths as a wide integer"""
    start, end = max(0, int(start)), max(0, int(end))
    if start + end > n:
        scale = F32(n) / F32(start + end)
        start = min(int(np.floor(F32(start) * scale)), n)
        end = min(int(np.floor(F32(end) * scale)), n)
    return start, end


def fade_tables(start, end, interp):
    """interp( float( frame ) / start ) and interp( float( frame ) / end ), :125 and :130; interp: fp32 -> fp32"""
    s = np.array([interp(F32(f) / F32(start)) for f in range(start)], F32)
    e = np.array([interp(F32(f) / F32(end)) for f in range(end)], F32)
    return s, e


def fade_frames(x, start, end, interp):
    """:102-135: the start's loop, then the end's, on a copy"""
    out = np.atleast_2d(x).astype(F32).copy()
    n = out.shape[1]
    start, end = fade_plan(n, start, end)
    s, e = fade_tables(start, end, interp)
    out[:, :start] = out[:, :start] * s
    if end:
        out[:, n - end:] = out[:, n - end:] * e[::-1]
    return out


def interp_sqrt(x):
    return np.sqrt(F32(x), dtype=F32)


def interp_linear(x):
    return F32(x)


# ---- waveforms (Function.cpp:32-39) ------------------------------------------------------------------------------------------------------
def waveform(kind, t):
    """fp32: fmod( t, 1.0f ), then the expression"""
    t0 = np.fmod(np.asarray(t, F32), F32(1.0)).astype(F32)
    if kind == SINE:
        return np.sin((PI2 * t0).astype(F32), dtype=F32)
    if kind == SQUARE:
        return np.where(t0 < F32(0.5), F32(-1.0), F32(1.0)).astype(F32)
    if kind == SAW:
        return (F32(-1.0) + F32(2.0) * t0).astype(F32)
    return np.where(t0 < F32(0.5), F32(-1.0) + F32(4.0) * t0, F32(3.0) - F32(4.0) * t0).astype(F32)


def waveform_truth(kind, t):
    """fp64 on the fp32 t"""
    t0 = np.fmod(np.asarray(t, np.float64), 1.0)
    if kind == SINE:
        return np.sin(np.float64(PI2) * t0)
    if kind == SQUARE:
        return np.where(t0 < 0.5, -1.0, 1.0)
    if kind == SAW:
        return -1.0 + 2.0 * t0
    return np.where(t0 < 0.5, -1.0 + 4.0 * t0, 3.0 - 4.0 * t0)


# ---- add_moisture's shaper (AudioVolume.cpp:179-187) --------------------------------------------------------------------------------------
def curve_index(F, sr_over, sr, n):
    """Frame( oversampled.frame_to_time( F ) * sr ) in fp32 (:161, :181-183), clamped to n - 1 (the stated deviation)"""
    t = (np.asarray(F).astype(F32) / F32(sr_over)).astype(F32)
    i = (t * F32(sr)).astype(F32).astype(np.int64)
    return np.minimum(np.maximum(i, 0), n - 1), i


def _at(curve, idx):
    curve = np.asarray(curve, F32)
    return curve[idx] if curve.ndim else np.full(np.shape(idx), curve, F32)


def moisture(s, F, sr_over, sr, n, amount, frequency, skew, kind=SINE, power32=None):
    """the fp32 restatement: every product an np.float32 product in the reference's order.  power32( |s|, skew ): the fp32 power, numpy's own
    unless given (numpy's vectorised powf is within an ulp, not exact even for an exponent of 1)"""
    s = np.asarray(s, F32)
    idx, _ = curve_index(F, sr_over, sr, n)
    a, fr, k = _at(amount, idx), _at(frequency, idx), _at(skew, idx)
    mag = np.power(np.abs(s), k, dtype=F32) if power32 is None else np.asarray(power32(np.abs(s), k), F32)
    power = np.where(s >= 0, mag, -mag).astype(F32)
    w = waveform(kind, ((PI2 * fr).astype(F32) * power).astype(F32))
    return (s + ((a * s).astype(F32) * w).astype(F32)).astype(F32)


def moisture_truth(s, F, sr_over, sr, n, amount, frequency, skew, kind=SINE):
    s64 = np.asarray(s, F32).astype(np.float64)
    idx, _ = curve_index(F, sr_over, sr, n)
    a, fr, k = (_at(c, idx).astype(np.float64) for c in (amount, frequency, skew))
    mag = np.power(np.abs(s64), k)
    power = np.where(s64 >= 0, mag, -mag)
    w = waveform_truth(kind, np.float64(PI2) * fr * power)
    return s64 + a * s64 * w


# ---- the oscillator's phases (AudioSynthesis.cpp:51-58) -----------------------------------------------------------------------------------
def phases_truth(freq, M):
    """the sequential fp64 modular sum of the fp32 frequencies, divided by M: phase[i] belongs to input frame i (an exclusive scan)"""
    freq = np.asarray(freq, F32).astype(np.float64)
    M = float(M)
    out = np.empty(freq.size, np.float64)
    p = 0.0
    for i, f in enumerate(freq.tolist()):
        out[i] = p / M
        p = math.fmod(p + f, M)
        if p < 0:
            p += M
    return out


def phases_fp32(freq, M):
    """the reference's operation in fp32, grouped sequentially (ONE of the groupings std::exclusive_scan may take)"""
    freq = np.asarray(freq, F32)
    M32 = F32(M)
    out = np.empty(freq.size, F32)
    p = F32(0.0)
    for i in range(freq.size):
        out[i] = F32(np.float64(p) / np.float64(M))          # :58: float /= double
        p = F32(np.fmod(F32(p + freq[i]), M32))
        if p < 0:
            p = F32(p + M32)
    return out


def circular_distance(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)) % 1.0
    return np.minimum(d, 1.0 - d)


def synthesize_waveform_frames(length, sr, oversample):
    """( num_frames, n_in, in_sample_rate ) of :33-44, None where the reference returns a null Audio"""
    if oversample < 1 or not length > 0 or not sr > 0:
        return None
    n = int(F32(length) * F32(sr))
    if n <= 0:
        return None
    return n, n * oversample, float(F32(sr) * F32(oversample))


# ---- energies ---------------------------------------------------------------------------------------------------------------------------
def energy_truth(x):
    """per channel: math.fsum of the exact squares (a product of two fp32 values is exact in fp64), then ONE rounding to fp32"""
    x = np.atleast_2d(x).astype(F32).astype(np.float64)
    with np.errstate(over="ignore"):
        return np.array([F32(math.fsum((row * row).tolist())) for row in x], F32)


def ulp(v):
    v = F32(abs(v))
    return float(np.spacing(v)) if np.isfinite(v) else 0.0


# ---- ADSR (Function.cpp:11-30) -----------------------------------------------------------------------------------------------------------
def adsr(t, a, d, s, r, level, a_exp=1.0, d_exp=1.0, r_exp=1.0):
    """one fp32 time -> one fp32 gain, every operation in fp32 in the reference's order"""
    t, a, d, s, r, level = (F32(v) for v in (t, a, d, s, r, level))
    a_exp, d_exp, r_exp = F32(a_exp), F32(d_exp), F32(r_exp)
    one = F32(1.0)
    with np.errstate(all="ignore"):
        if t < 0 or t > F32(F32(F32(a + d) + s) + r):
            return F32(0.0)
        if t < a:
            return np.power(F32(t / a), a_exp, dtype=F32)
        if t < F32(a + d):
            return F32(F32(np.power(F32(one - F32(F32(t - a) / d)), d_exp, dtype=F32) * F32(one - level)) + level)
        if t < F32(F32(a + d) + s):
            return level
        if t < F32(F32(F32(a + d) + s) + r):
            return F32(np.power(F32(one - F32(F32(F32(F32(t - a) - d) - s) / r)), r_exp, dtype=F32) * level)
    return F32(0.0)


# ---- white noise (AudioSynthesis.cpp:80-86) ------------------------------------------------------------------------------------------------
def white_noise_draw(seed, count):
    """std::mt19937( seed ) through std::uniform_real_distribution<>( -1.0f, 1.0f ) as libstdc++ draws it: generate_canonical< double, 53 > takes
    two engine outputs, ( lo + hi * 2^32 ) / 2^64 in double (1 - 2^-53 if that rounds to 1), times ( b - a ) plus a; narrowed to fp32"""
    g = MT19937(seed)
    out = np.empty(count, F32)
    for i in range(count):
        lo, hi = float(g()), float(g())
        c = (lo + hi * 4294967296.0) / 18446744073709551616.0
        if c >= 1.0:
            c = 1.0 - 2.0 ** -53
        out[i] = F32(c * 2.0 + -1.0)
    return out


# ---- get_amplitude_envelope (AudioInformation.cpp:320-363) ---------------------------------------------------------------------------------
def mono(x):
    """convert_to_mono: the channels added in order in fp32, divided by their number"""
    x = np.atleast_2d(x).astype(F32)
    acc = x[0].copy()
    for c in range(1, x.shape[0]):
        acc = (acc + x[c]).astype(F32)
    return (acc / F32(x.shape[0])).astype(F32)


def rectify(x):
    x = np.asarray(x, F32)
    return np.where(x < 0, x * F32(-1.0), x).astype(F32)


def hann_window(width_frames):
    """( window, the fp32 running sum ) of :337-343; width_frames: the fp32 time_to_frame( window_width ).  Windows::hann takes the fp32
    argument 2.0f * pi * x into the DOUBLE cos and narrows on return"""
    width_frames = F32(width_frames)
    count = int(width_frames)
    w = np.empty(count, F32)
    total = F32(0.0)
    for i in range(count):
        x = F32(F32(i) / F32(width_frames - F32(1.0)))
        w[i] = F32(0.5 * (1.0 - math.cos(float(F32(F32(F32(2.0) * PI) * x)))))
        total = F32(total + w[i])
    return w, total


def envelope_gain(total):
    return F32(F32(PI / F32(2.0)) / F32(total))          # :346


def envelope_function(ys, sr, t):
    """:351-363 at one fp32 time"""
    ys = np.asarray(ys, F32)
    x = F32(F32(t) * F32(sr))
    if 0 <= x < ys.size - 1:
        x1 = int(np.floor(x))
        return F32(ys[x1] + F32(F32(ys[x1 + 1] - ys[x1]) * F32(x - F32(x1))))
    return F32(0.0)
