"""A numpy restatement of the reference's sliding-DFT vocoder (Conversions/AudioSPV.cpp) in its fp32 order, and an fp64 truth.

Line numbers cite Conversions/AudioSPV.cpp.  Every complex product is written on separate float32 real and imaginary arrays, one
ufunc per operation, so that neither FMA contraction nor a complex64 loop changes the rounding.  phase_vocoder / inverse_phase_vocoder
are the reference's own translation units (oracle/_ref/libflanref.so through oracle_lib.load_ref()).

N = num_bins, L = 2 N.  The identity behind the GPU design: the running sum of stage 3 telescopes to
S[f][b] = T[(f+1) b] D_f[b], D_f the L-point DFT of the window x[f-L+1 .. f], so the demodulated F[f][b] = D_f[b].
"""
import ctypes as C

import numpy as np

import oracle_lib as O

F32 = np.float32
PI2 = F32(6.2831854820251465)          # defines.h: pi2 = acos(-1.0f) * 2.0f

_libm = C.CDLL("libm.so.6")
_libm.cosf.restype = C.c_float
_libm.cosf.argtypes = [C.c_float]
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]


def twiddles(N):
    """:13-22, :37-38: T[i] = std::polar( 1.0f, omega * i ), omega = -pi2 / L in float -> (re, im) float32 [L] each."""
    L = 2 * N
    omega = F32(-PI2) / F32(L)
    theta = (omega * np.arange(L, dtype=F32)).astype(F32)
    re = np.array([_libm.cosf(float(t)) for t in theta], F32)
    im = np.array([_libm.sinf(float(t)) for t in theta], F32)
    return re, im


def _ref():
    ref = O.load_ref()
    if ref is None:
        raise RuntimeError("oracle/_ref/libflanref.so is not built")
    return ref


def running_sums(x, N, T=None):
    """Stages 2-3 (:45-58) for one channel: S[f][b] as float32 (re, im) [n][N]."""
    n = x.shape[0]
    L = 2 * N
    Tr, Ti = T if T is not None else twiddles(N)
    x = x.astype(F32)
    xo = np.zeros(n, F32)
    if n > L:
        xo[L:] = x[:n - L]
    d = (x - xo).astype(F32)                                        # :50
    b = np.arange(N, dtype=np.int64)
    Sr = np.empty((n, N), F32)
    Si = np.empty((n, N), F32)
    Sr[0] = d[0]                                                    # :56
    Si[0] = F32(0)
    for f in range(1, n):                                           # :57-58
        k = (f * b) % L
        Sr[f] = Sr[f - 1] + d[f] * Tr[k]
        Si[f] = Si[f - 1] + d[f] * Ti[k]
    return Sr, Si


def demodulate_hann(Sr, Si, N, T=None, frames=None):
    """Stage 4 (:61-92): F = S conj( T[((f+1) b) % L] ), then the 3-tap with the edge rule, / float( L ).  frames: the frame numbers
    of the rows of Sr / Si (default 0 .. n-1)."""
    L = 2 * N
    Tr, Ti = T if T is not None else twiddles(N)
    f = np.arange(Sr.shape[0], dtype=np.int64) if frames is None else np.asarray(frames, np.int64)
    k = ((f[:, None] + 1) * np.arange(N, dtype=np.int64)[None, :]) % L
    cr, ci = Tr[k], -Ti[k]
    Fr = Sr * cr - Si * ci
    Fi = Sr * ci + Si * cr
    ar, ai = Fr + Fr, Fi + Fi
    br = np.empty_like(Fr)
    bi = np.empty_like(Fi)
    br[:, 1:N - 1] = Fr[:, 0:N - 2] + Fr[:, 2:N]
    bi[:, 1:N - 1] = Fi[:, 0:N - 2] + Fi[:, 2:N]
    br[:, 0] = Fr[:, 1] * F32(2)                                    # :68-69 bin 0: complex( 2 Re F[1], 0 )
    bi[:, 0] = F32(0)
    br[:, N - 1] = Fr[:, N - 2] * F32(2)                            # :86-88 bin N-1: complex( 2 Re F[N-2], 0 )
    bi[:, N - 1] = F32(0)
    vr = (F32(0.25) * (ar - br)) / F32(L)
    vi = (F32(0.25) * (ai - bi)) / F32(L)
    return vr.astype(F32), vi.astype(F32)


def bin_frequencies(N, sr):
    """SPVBuffer::bin_to_frequency( b ) = b * sr / N in float."""
    return (np.arange(N, dtype=F32) * F32(sr) / F32(N)).astype(F32)


def vocode(vr, vi, N, sr):
    """Stage 5 (:94-102): phase_vocoder per bin over the frames, analysis rate = sample rate, phase buffer from 0."""
    ref = _ref()
    n = vr.shape[0]
    bf = bin_frequencies(N, sr)
    ph = np.zeros(N, np.float64)
    m = np.empty((n, N), F32)
    fr = np.empty((n, N), F32)
    for f in range(n):
        rr = np.ascontiguousarray(vr[f])
        ii = np.ascontiguousarray(vi[f])
        mm = np.empty(N, F32)
        ff = np.empty(N, F32)
        ref.ref_phase_vocoder_batch(N, ph, rr, ii, bf, F32(sr), F32(sr), mm, ff)
        m[f], fr[f] = mm, ff
    return m, fr


def analyze(audio, sr, N):
    """Audio::convert_to_SPV( N ): float32 [ch][n] -> float32 [ch][n][N][2] (m, f)."""
    audio = np.atleast_2d(np.asarray(audio, F32))
    T = twiddles(N)
    out = np.empty(audio.shape + (N, 2), F32)
    for c in range(audio.shape[0]):
        Sr, Si = running_sums(audio[c], N, T)
        vr, vi = demodulate_hann(Sr, Si, N, T)
        out[c, :, :, 0], out[c, :, :, 1] = vocode(vr, vi, N, sr)
    return out


def synthesize(spv, sr):
    """SPV::convert_to_audio (:110-145): inverse_phase_vocoder per bin from 0, then sample = 2 sum_b (-1)^b Re, fp32 in bin order."""
    ref = _ref()
    spv = np.asarray(spv, F32)
    ch, n, N, _ = spv.shape
    out = np.empty((ch, n), F32)
    sign = np.where(np.arange(N) % 2 == 0, F32(1), F32(-1)).astype(F32)
    for c in range(ch):
        ph = np.zeros(N, np.float64)
        re = np.empty((n, N), F32)
        for f in range(n):
            m = np.ascontiguousarray(spv[c, f, :, 0])
            fr = np.ascontiguousarray(spv[c, f, :, 1])
            rr = np.empty(N, F32)
            ii = np.empty(N, F32)
            ref.ref_inverse_phase_vocoder_batch(N, ph, m, fr, F32(sr), rr, ii)
            re[f] = rr
        terms = (re * sign[None, :]).astype(F32)
        acc = np.zeros(n, F32)
        for b in range(N):                                          # :137-138, in bin order
            acc = acc + terms[:, b]
        out[c] = acc * F32(2)
    return out


def truth_spectra(x, N, frames):
    """fp64 complex values after the 3-tap and / L at `frames`: [len(frames)][N] (see truth)."""
    x = np.asarray(x, np.float64)
    L = 2 * N
    rows = []
    for f in frames:
        w = np.zeros(L)
        lo = f - L + 1
        seg = x[max(lo, 0):f + 1]
        w[L - len(seg):] = seg
        D = np.fft.fft(w)[:N]                                        # D_f[b] = sum_k w[k] exp( -2 pi i k b / L )
        a = 2.0 * D
        bb = np.empty(N, complex)
        bb[1:N - 1] = D[0:N - 2] + D[2:N]
        bb[0] = 2.0 * D[1].real
        bb[N - 1] = 2.0 * D[N - 2].real
        rows.append(0.25 * (a - bb) / L)
    return np.array(rows)


def truth(x, N, sr, frames):
    """fp64 "truth" at the given frames of one channel: np.fft of the trailing window (x[f-L+1 .. f], zeros before the start), the same
    3-tap and edge rule, / L; magnitude and the fp64 phase.  Returns (m, phase) float64 [len(frames)][N]; the frequency of frame f
    is (phase[f] - phase[f-1]) * sr / 2 pi, so ask for consecutive pairs."""
    V = truth_spectra(x, N, frames)
    return np.abs(V), np.angle(V)


def truth_frequency(x, N, sr, frames):
    """fp64 m and f at `frames` (each >= 1): phase_vocoder without wrapping, f = dphase * sr / 2 pi with dphase in (-2 pi, 2 pi) as
    atan2 differences are."""
    frames = np.asarray(frames, np.int64)
    both = np.concatenate([frames - 1, frames])
    m, ph = truth(x, N, sr, both)
    k = len(frames)
    dph = ph[k:] - ph[:k]
    return m[k:], dph * sr / (2.0 * np.pi)


def p1_metrics(pv_gpu, pv_ref, analysis_rate, real_edges=False):
    """rel_m, m^2-weighted rms of the frequency difference (whole turns of analysis_rate folded out), the bit-identical fraction of f
    over the significant bins, and the count of folded turns there -- the P1 statistics of the PV tests, restated.
    real_edges (the SPV): bins 0 and N-1 hold real values by construction (AudioSPV.cpp:66-69, :86-88; the imaginary part is +-0), so
    their phase is 0 or pi and a value within rounding of zero that takes the other sign moves f by half a turn, analysis_rate / 2:
    there half turns are folded out (and counted) as well."""
    m_g, f_g = pv_gpu[..., 0].astype(np.float64), pv_gpu[..., 1].astype(np.float64)
    m_r, f_r = pv_ref[..., 0].astype(np.float64), pv_ref[..., 1].astype(np.float64)
    rel_m = np.sqrt(np.sum((m_g - m_r) ** 2) / max(np.sum(m_r ** 2), 1e-300))
    df = f_g - f_r
    turns = np.rint(df / analysis_rate)
    df_folded = df - turns * analysis_rate
    if real_edges:
        for b in (0, df.shape[-1] - 1):
            half = np.rint(df[..., b] / (0.5 * analysis_rate))
            df_folded[..., b] = df[..., b] - half * (0.5 * analysis_rate)
            turns[..., b] = half
    w = m_r ** 2
    wrms_f = np.sqrt(np.sum(w * df_folded ** 2) / max(np.sum(w), 1e-300))
    sig = m_r > 1e-4 * max(m_r.max(), 1e-300)
    eq = pv_gpu[..., 1].view(np.uint32) == pv_ref[..., 1].view(np.uint32)
    same = float(np.mean(eq[sig])) if sig.any() else 1.0
    return rel_m, wrms_f, same, int(np.count_nonzero(turns[sig]))
