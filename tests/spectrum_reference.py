"""Audio::synthesize_spectrum (Audio/AudioSynthesis.cpp:151-268) restated in NumPy: the per-bin harmonics and magnitudes in the reference's fp32
arithmetic, the phases of std::mt19937, the table as the unnormalised c2r (an fp64 truth and a single-precision stand-in), the channel jumps
and the resampler loop, which is wavetable_reference.synth over the rotated table.  What the tests of flan_amd/csrc/spectrum.hip compare with.

Bins the reference skips ( harmonic == 0 ) are ZERO here, as in the library (the reference leaves them uninitialised)."""
import os

import numpy as np

import wavetable_reference as WT

F32 = np.float32
RATE = F32(48000.0)
PI2 = F32(np.arccos(F32(-1.0))) * F32(2.0)          # defines.h: pi = std::acos( -1.0f ), pi2 = pi * 2.0f
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_made", "wdl_spectrum.npz")


def sizes(p):
    """( N, C, B ) of spectrum_size_power p"""
    N = 1 << p
    return N, N // 2, N // 2 + 1


def bins(p, fundamental_power):
    """( int32 harmonic[B], float32 freq[B] ): bin_to_frequency( b ) = b * 48000 / float( B ) (:186 -- by the number of bins, not N) and
    harmonic = int( round( freq / fundamental ) ) (:201; std::round, halves away from zero)"""
    _, _, B = sizes(p)
    freq = ((np.arange(B).astype(F32) * RATE).astype(F32) / F32(B)).astype(F32)
    q = (freq / F32(2.0 ** fundamental_power)).astype(F32)
    return np.floor(q.astype(np.float64) + 0.5).astype(np.int32), freq


def num_harmonics(fundamental_power):
    """ceil( bin_to_frequency( B ) / fundamental ) + 1 with bin_to_frequency( B ) = 48000 (:188)"""
    return int(np.ceil(RATE / F32(2.0 ** fundamental_power))) + 1


def gaussian(x):
    """the default peak_distribution (Audio.h): 1.0f / std::sqrt( pi2 ) * std::exp( -0.5f * std::pow( x, 2.0f ) ), in fp32"""
    x = np.asarray(x, F32)
    return ((F32(1.0) / np.sqrt(PI2)) * np.exp((F32(-0.5) * (x * x).astype(F32)).astype(F32)).astype(F32)).astype(F32)


def default_spread(h):
    """Audio.h: []( Harmonic h ){ return h; }"""
    return F32(h)


def default_harmonic_scale(h):
    """Audio.h: []( Harmonic h ){ return 1.0f / std::sqrt( h ); } -- the square root of an int is a double"""
    return F32(1.0 / np.sqrt(np.float64(h)))


def magnitudes(p, fundamental_power, spread=default_spread, harmonic_scale=default_harmonic_scale, distribution=gaussian):
    """float32 mag[B] (:198-210).  spread, harmonic_scale: functions of the harmonic number, sampled once per harmonic 1 ... num_harmonics;
    r = ( sd <= 0.001 ? x : distribution( ( x - mean ) / sd ) / sd ) * harmonic_scale( harmonic ), 0 where harmonic == 0"""
    harmonic, freq = bins(p, fundamental_power)
    nh = num_harmonics(fundamental_power)
    hs = np.array([harmonic_scale(h) for h in range(1, nh + 1)], F32)
    sp = np.array([spread(h) for h in range(1, nh + 1)], F32)
    on = harmonic != 0
    h = np.where(on, harmonic, 1)
    mean = (F32(2.0 ** fundamental_power) * h.astype(F32)).astype(F32)
    sd = sp[h - 1]
    flat = sd <= F32(0.001)
    safe = np.where(flat, F32(1.0), sd)
    peak = (distribution(((freq - mean).astype(F32) / safe).astype(F32)).astype(F32) / safe).astype(F32)
    r = (np.where(flat, freq, peak).astype(F32) * hs[h - 1]).astype(F32)
    return np.where(on, r, F32(0.0)).astype(F32)


def phases(seed, harmonic):
    """std::mt19937( seed ) and one std::uniform_real_distribution<float>( 0, 2 pi ) draw per bin with a harmonic, ascending; 0 elsewhere.
    libstdc++: generate_canonical<float, 24> takes one 32-bit word w, float( w ) * 2^-32 (the value below 1 if that rounds to 1), times 2 pi"""
    harmonic = np.asarray(harmonic)
    bg = np.random.MT19937()
    bg._legacy_seeding(int(seed))                   # init_genrand( seed ): std::mt19937's seeding
    on = harmonic != 0
    raw = bg.random_raw(int(np.count_nonzero(on)))
    u = (raw.astype(F32) * F32(2.0 ** -32)).astype(F32)
    u = np.where(u >= F32(1.0), np.nextafter(F32(1.0), F32(0.0)), u).astype(F32)
    theta = np.zeros(harmonic.size, F32)
    theta[on] = (u * PI2).astype(F32)
    return theta


def table_truth(mag, theta):
    """float64 table[N]: fp64 inputs from the fp32 mag / theta (X = polar( r, theta ) in fp64), then the unnormalised c2r, which ignores the
    imaginary parts of bins 0 and C"""
    import scipy.fft as sf
    mag, theta = np.asarray(mag, F32).astype(np.float64), np.asarray(theta, F32).astype(np.float64)
    N = 2 * (mag.size - 1)
    return sf.irfft(mag * np.exp(1j * theta), N) * N


def table_standin(mag, theta):
    """the same through scipy.fft in single precision (pocketfft keeps complex64 -> float32)"""
    import scipy.fft as sf
    mag, theta = np.asarray(mag, F32).astype(np.float64), np.asarray(theta, F32).astype(np.float64)
    N = 2 * (mag.size - 1)
    y = sf.irfft((mag * np.exp(1j * theta)).astype(np.complex64), N)
    assert y.dtype == F32
    return (y * F32(N)).astype(F32)


def table_direct(mag, theta):
    """the O( N^2 ) sum of the c2r's definition in fp64:
    table[n] = Re X0 + (-1)^n Re X_C + 2 sum_{k=1}^{C-1} Re( X_k exp( +2 pi i k n / N ) )"""
    mag, theta = np.asarray(mag, F32).astype(np.float64), np.asarray(theta, F32).astype(np.float64)
    C = mag.size - 1
    N = 2 * C
    X = mag * np.exp(1j * theta)
    n = np.arange(N)
    k = np.arange(1, C)
    inner = 2.0 * np.real(np.exp(2j * np.pi * ((k[None, :] * n[:, None]) % N) / N) @ X[1:C])
    return X[0].real + np.where(n % 2 == 0, 1.0, -1.0) * X[C].real + inner


def jump(channel, num_channels, p):
    """Frame( ( float( channel ) / num_channels ) * N ) (:236)"""
    return int((F32(channel) / F32(num_channels)) * F32(1 << p))


def synth_plan(out_frames, fundamental, g, freq):
    """the block plan: Wavetable::synthesize's with rate_out = max( fundamental, 1 ) in place of sr / W (a wavelength of 1 frame gives it);
    it does not depend on the channel or on the table's size"""
    return WT.synth_plan(out_frames, float(fundamental), 1, g, freq)


def synth(table, fundamental, num_channels, out_frames, g, freq):
    """the loop of :230-263: float32 [num_channels][out_frames].  Channel c is Wavetable::synthesize over the table rotated by its jump:
    one slot, no blend, sr = fundamental * N"""
    table = np.asarray(table, F32).reshape(-1)
    N = table.size
    p = N.bit_length() - 1
    sr = F32(fundamental) * F32(N)
    assert float(sr) == float(fundamental) * N and float(sr) / N == float(fundamental)
    blocks = WT.synth_plan(out_frames, sr, N, g, freq)
    index = np.zeros((1, len(blocks)), F32)
    rows = [WT.synth(np.roll(table, -jump(c, num_channels, p))[None], N, sr, out_frames, g, freq, index, smooth=False, blocks=blocks)[0]
            for c in range(num_channels)]
    return np.array(rows, F32)


def set_volume(audio, level=1.0, sr=48000.0):
    """Audio::set_volume (AudioVolume.cpp:46-67) with a scalar level: audio * ( level / m ), m the max |sample| over frames [0, end) --
    end = clamp( Frame( float( N ) / sr * sr ), 0, N - 1 ), so the last frame is not looked at --; m == 0 hands the input through"""
    audio = np.asarray(audio, F32)
    n = audio.shape[1]
    end = min(max(int((F32(n) / F32(sr)) * F32(sr)), 0), n - 1)
    m = F32(np.max(np.abs(audio[:, :end]))) if end > 0 else F32(0.0)
    if m == 0:
        return audio.copy(), end
    return (audio * (F32(level) / m)).astype(F32), end


def golden_table(p):
    """the fixture's table: ( ( ( i * 2654435761 mod 2^32 ) >> 8 ) / 2^24 - 0.5 ) in fp32"""
    i = np.arange(1 << p, dtype=np.uint64)
    w = ((i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)
    return (w.astype(F32) / F32(2.0 ** 24) - F32(0.5)).astype(F32)


def load_cases():
    """the reference-made fixture as a list of dicts"""
    z = np.load(GOLDEN)
    cases = []
    for k, name in enumerate(z["names"]):
        p, fundamental, ch, g, nout, blocks = z["meta_%d" % k]
        cases.append(dict(name=str(name), table=z["table_%d" % k], freq=z["freq_%d" % k], p=int(p), fundamental=float(fundamental), ch=int(ch),
                          g=int(g), out_frames=int(nout), blocks=int(blocks), out=z["out_%d" % k], wanted=z["wanted_%d" % k],
                          delivered=z["delivered_%d" % k]))
    return cases
