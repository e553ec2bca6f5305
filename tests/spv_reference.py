"""A numpy restatement of the reference's sliding-DFT vocoder (Conversions/AudioSPV.cpp) in its fp32 order, and an fp64 truth.

Line numbers cite Conversions/AudioSPV.cpp.  Every complex product is written on separate float32 real and imaginary arrays, one
ufunc per operation, so that neither FMA contraction nor a complex64 loop changes the rounding.  phase_vocoder / inverse_phase_vocoder
are the reference's own translation units (oracle/_ref/libflanref.so through oracle_lib.load_ref()).

N = num_bins, L = 2 N.  The identity behind the GPU design: the running sum of stage 3 telescopes to
S[f][b] = T[(f+1) b] D_f[b], D_f the L-point DFT of the window x[f-L+1 .. f], so the demodulated F[f][b] = D_f[b].

The synthesis is restated twice: synthesize() runs the reference's own inverse_phase_vocoder (oracle/_ref), synthesize_np() needs nothing
but numpy (inverse_phases() is phase_vocoder.cpp:55-61 in fp64, vectorised over bins), and synthesis_truth() is its fp64 truth.  SYN_CASES
is the case table of tests/test_gpu_spv_synthesis.py, built here so that tests/test_spv_reference.py can print the restatement's own error
on every case without a GPU.
"""
import ctypes as C
import functools

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


def running_sums(x, N, T=None, keep=None):
    """Stages 2-3 (:45-58) for one channel: S[f][b] as float32 (re, im) [n][N]; with keep (frame numbers), only those rows, in keep's order."""
    if keep is not None:
        return _running_sums_at(x, N, T if T is not None else twiddles(N), np.asarray(keep, np.int64))
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


def _running_sums_at(x, N, T, keep):
    n = x.shape[0]
    L = 2 * N
    Tr, Ti = T
    x = x.astype(F32)
    xo = np.zeros(n, F32)
    if n > L:
        xo[L:] = x[:n - L]
    d = (x - xo).astype(F32)
    b = np.arange(N, dtype=np.int64)
    rows = {}
    wanted = set(int(f) for f in keep)
    sr_ = np.full(N, d[0], F32)
    si_ = np.zeros(N, F32)
    if 0 in wanted:
        rows[0] = (sr_, si_)
    for f in range(1, n):
        k = (f * b) % L
        sr_ = sr_ + d[f] * Tr[k]
        si_ = si_ + d[f] * Ti[k]
        if f in wanted:
            rows[f] = (sr_, si_)
    return np.stack([rows[int(f)][0] for f in keep]), np.stack([rows[int(f)][1] for f in keep])


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


def analyze_frames(x, sr, N, frames):
    """The rows `frames` (each >= 1) of analyze() for one channel, float32 [len(frames)][N][2], without holding every frame: the running
    sum walks the whole channel, the demodulation and phase_vocoder run at frames - 1 (whose phase is `prev`) and at frames only."""
    ref = _ref()
    x = np.asarray(x, F32)
    frames = np.asarray(frames, np.int64)
    T = twiddles(N)
    both = np.concatenate([frames - 1, frames])
    Sr, Si = running_sums(x[:int(both.max()) + 1], N, T, keep=both)
    vr, vi = demodulate_hann(Sr, Si, N, T, frames=both)
    bf = bin_frequencies(N, sr)
    k = len(frames)
    out = np.empty((k, N, 2), F32)
    for i in range(k):
        ph = np.zeros(N, np.float64)
        mm, ff = np.empty(N, F32), np.empty(N, F32)
        for row in (i, k + i):
            ref.ref_phase_vocoder_batch(N, ph, np.ascontiguousarray(vr[row]), np.ascontiguousarray(vi[row]), bf, F32(sr), F32(sr), mm, ff)
        out[i, :, 0], out[i, :, 1] = mm, ff
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


def inverse_phases(f, ar, phase0=None):
    """The recurrence of inverse_phase_vocoder (phase_vocoder.cpp:57-59) for every frame of f [..., n, N] float32, per bin from phase0
    (default 0): pd = float( float( f / ar ) * pi2 ); phase += double( pd ); if( phase > pi2 ) phase = fmod( phase, pi2 ), pi2 the FLOAT's
    value as a double.  Each fold therefore moves the angle by 2 pi - pi2 = -1.7e-7 rad, a negative phase is never folded, and fmod of
    +inf is NaN: all of it is the definition.  Returns the phase after each frame, float64 [..., n, N]."""
    f = np.asarray(f, F32)
    n = f.shape[-2]
    P = float(PI2)
    out = np.empty(f.shape, np.float64)
    ph = np.zeros(f.shape[:-2] + f.shape[-1:], np.float64) if phase0 is None else np.array(phase0, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pd = ((f / F32(ar)).astype(F32) * PI2).astype(F32)
        for i in range(n):
            ph = ph + pd[..., i, :].astype(np.float64)
            ph = np.where(ph > P, np.fmod(ph, P), ph)
            out[..., i, :] = ph
    return out


def cos_f32(x):
    """cos of float32 angles, correctly rounded to float32 (through fp64): within one ulp of any libm's cosf, with no table of its own"""
    with np.errstate(invalid="ignore"):
        return np.cos(np.asarray(x, F32).astype(np.float64)).astype(F32)


def _signs(N):
    return np.where(np.arange(N) % 2 == 0, F32(1), F32(-1)).astype(F32)


def synthesize_np(spv, ar, phases=None):
    """SPV::convert_to_audio restated in numpy alone: re = float( m cosf( float( phase ) ) ) (std::polar( m, float( phase ) ).real()),
    sign (-1)^b, an fp32 sum in bin order, * 2 (AudioSPV.cpp:137-140).  float32 [ch][n]."""
    spv = np.asarray(spv, F32)
    ch, n, N, _ = spv.shape
    ph = inverse_phases(spv[..., 1], ar) if phases is None else phases
    with np.errstate(invalid="ignore"):
        re = (spv[..., 0] * cos_f32(ph.astype(F32))).astype(F32)
        terms = (re * _signs(N)).astype(F32)
        acc = np.zeros((ch, n), F32)
        for b in range(N):
            acc = acc + terms[:, :, b]
        return (acc * F32(2)).astype(F32)


def synthesis_truth(spv, ar, phases=None):
    """The same phases and the same float( phase ) rounding (both are the definition); cos, product and sum in fp64.  float64 [ch][n]."""
    spv = np.asarray(spv, F32)
    N = spv.shape[2]
    ph = inverse_phases(spv[..., 1], ar) if phases is None else phases
    with np.errstate(invalid="ignore"):
        terms = spv[..., 0].astype(np.float64) * np.cos(ph.astype(F32).astype(np.float64)) * _signs(N).astype(np.float64)
        return 2.0 * np.sum(terms, axis=-1)


def synthesis_errors(got, want):
    """rms( got - want ) / rms( want ) and max | got - want | / max | want |"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    d = got - want
    return float(np.sqrt(np.mean(d ** 2) / np.mean(want ** 2))), float(np.max(np.abs(d)) / np.max(np.abs(want)))


# ---------------------------------------------------------------------------------------------------------------------------------
# The synthesis case table.  cut: frames per chain forced through fa.spv_chain_length (None: the library's own).  regime: which
# bound against the restatement applies.  kind: how f is drawn (spv_case).  m is 10^U[-3, 0] throughout.
# ---------------------------------------------------------------------------------------------------------------------------------

def _c(name, N, ch, n, cut, kind, regime="uniform", sr=48000.0):
    return dict(name=name, N=N, ch=ch, n=n, cut=cut, kind=kind, regime=regime, sr=sr)


SYN_CASES = (
    # every register variant of k_spv_synthesize (K = 1, 2, 4, 8, 16, 0), full and ragged last columns
    [_c("bins%d" % N, N, 1, 75, 32, "uniform") for N in (2, 3, 255, 256, 257, 512, 513, 1025, 2049, 4096, 4097)]
    + [_c("channels", 300, 3, 203, 64, "uniform")]
    # one chain (the memset path), last batches of 1 .. 32 frames; 129: the library's first two-chain length
    + [_c("one_chain_N%d_n%d" % (N, n), N, 2, n, None, "uniform") for N in (7, 300) for n in (1, 31, 32, 33, 127, 128)]
    + [_c("two_chains_N%d" % N, N, 2, 129, None, "uniform") for N in (7, 300)]
    # the scan's batches of 16 loads: chains on both sides of 16 and of 32, a last chain of 27 frames
    + [_c("scan%d" % k, 5, 2, 32 * k - 5, 32, "uniform") for k in (2, 15, 16, 17, 18, 32, 33)]
    + [_c("one_frame_chains", 5, 1, 50, 1, "uniform")]
    + [_c("negative", 300, 1, 700, 96, "negative", "negative")]
    + [_c("wide", 300, 1, 300, 64, "wide", "wide")]
    + [_c("sincos_wide", 40, 1, 200, 64, "held", "extreme")]
    + [_c("fold_any", 40, 1, 200, 64, "huge", "extreme")]
    + [_c("rate%d" % sr, 300, 1, 203, 64, "uniform", sr=float(sr)) for sr in (8000, 44100, 192000)]
    # phases that walk at random on both sides of 0 (steps of up to +-7.9 rad): the reference folds a bin only while it is above pi2, and
    # holds whatever negative phase it has reached, -355 rad here
    + [_c("wander", 300, 1, 700, 32, "wander", "wide")]
)
SYN_IDS = [c["name"] for c in SYN_CASES]
HUGE_F = (2.5e13, 1e20)          # f / 48000 * pi2 = 3.3e9 and 1.3e16 rad a frame: past fold_phase_fast's 3e9


def syn_case(name):
    return next(c for c in SYN_CASES if c["name"] == name)


@functools.lru_cache(maxsize=None)
def spv_case(name):
    """The case's SPV, float32 [ch][n][N][2], read-only; built in numpy, never taken from the analysis."""
    c = syn_case(name)
    N, ch, n, sr = c["N"], c["ch"], c["n"], c["sr"]
    rng = np.random.default_rng(SYN_IDS.index(name) + 1)
    spv = np.empty((ch, n, N, 2), F32)
    spv[..., 0] = 10.0 ** rng.uniform(-3.0, 0.0, (ch, n, N))
    lo, hi = {"negative": (-3000.0, 500.0), "wide": (-24000.0, 96000.0), "wander": (-60000.0, 60000.0)}.get(c["kind"], (0.0, 0.5 * sr))
    spv[..., 1] = rng.uniform(lo, hi, (ch, n, N))
    if c["kind"] == "held":          # | float( phase ) | passes 2^22 at frame 33: sincos_fast before, sincos_wide after
        spv[:, :, rng.choice(N, 10, replace=False), 1] = F32(-1e9)
    if c["kind"] == "huge":
        at = rng.choice(n * N, 20, replace=False)
        spv[0].reshape(n * N, 2)[at, 1] = np.repeat(np.array(HUGE_F, F32), 10)
    spv.setflags(write=False)
    return spv


@functools.lru_cache(maxsize=None)
def syn_expected(name):
    """(restatement float32 [ch][n], truth float64 [ch][n]) of a case, computed once, read-only"""
    c, spv = syn_case(name), spv_case(name)
    ph = inverse_phases(spv[..., 1], c["sr"])
    want, truth = synthesize_np(spv, c["sr"], ph), synthesis_truth(spv, c["sr"], ph)
    want.setflags(write=False)
    truth.setflags(write=False)
    return want, truth


def truth_spv(x, N, sr):
    """An SPV like an analysis': the fp64 truth's m and f at every frame (frame 0 from a zero phase), rounded to float32.  The stand-in
    for the device analysis where there is no device."""
    x = np.atleast_2d(np.asarray(x, np.float64))
    ch, n = x.shape
    out = np.empty((ch, n, N, 2), F32)
    for c in range(ch):
        V = truth_spectra(x[c], N, np.arange(n))
        ph = np.angle(V)
        dph = np.diff(ph, axis=0, prepend=np.zeros((1, N)))
        out[c, :, :, 0] = np.abs(V)
        out[c, :, :, 1] = dph * sr / (2.0 * np.pi)
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
