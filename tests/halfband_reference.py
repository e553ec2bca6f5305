"""hilbert_phase_diff_network (Audio/AudioFilter.cpp:1045-1160), Audio::halfband_modulate (:1162-1186), Audio::shift_frequency (:1188-1227)
and Audio::halfband_multiply (:1229-1263) restated in NumPy.  DESIGN.md 4.17.

    poles()                  phase_diff_network_pole_design( 20, 5, 22000 ) in fp64, each pole rounded to fp32: ( first, second )
    coefficients( sr )       G [2][10] in fp32: T_half = pi / sr, g = p T_half, G = g / ( 1 + g ) -- no prewarp, no clamp
    network()                the sequential loop over the frames, every frame through a cascade's ten sections (:61-80 with the mix
                             { 1, -1 }), in fp32 with one rounding per operation, or in fp64 from the SAME fp32 G (the "truth")
    state_space( G )         the cascade as s' = A s + b x, y = c s + d x with A lower triangular: the algebra of halfband.hip
    response( sr, hz )       the cascades' frequency responses from the same G, in fp64
    combine()                first * re - second * im, the product of halfband_modulate and halfband_multiply
    shift_curves(), shift_frequency()
    errors(), CASES

cos and sin of the phase are the fp64 functions of the fp32 phase rounded to fp32 once: what the device kernels do."""
import functools

import numpy as np

import filter_reference as R1

F32, F64 = np.float32, np.float64
K = 10                                                  # sections of one cascade
PI = R1.PI                                              # defines.h: acosf( -1 ), a float
PI2 = PI * F32(2)
TRUTH_FACTOR = 4.0                                      # filter2_reference's truth criterion: at most 4 x the restatement's own error on
TRUTH_FLOOR = 8 * 2.0 ** -23                            # the same case, or 8 fp32 ulps of the input's scale
# What the device is held to against the fp32 restatement: rms( got - want ) / rms( x ) and max | got - want | / max | x | (multiply: the
# products of the two operands' rms and peaks).  These cannot be derived; they are TWICE the worst the MI355X measured over CASES and the
# five results (hilbert's two outputs, modulate with rows, modulate with a phase row, multiply), the factor 2 for the run lengths and boxes
# that filter2_reference's bounds also absorb.  One pair per kind of input, because the kinds differ by two orders of magnitude and one
# pair for all would hold noise to the step's figures: on a DC step the sequential fp32 loop itself drifts from the truth (3.97e-5 rms after
# 9001 frames: the slowest sections add G ( x - s ) with G of 6e-4 to a state that has all but arrived), while the device, whose start
# states come from the fp64 scan every 16 frames, stays 1.4e-7 from the truth -- there the distance to the restatement IS the
# restatement's error, and the truth criterion is the one that binds.
MEASURED = {                                            # kind: ( rel_rms, rel_max ), the worst case and result of the kind
    "noise": (1.061e-06, 3.864e-06),                    # n8192_c3_noise_48_run0 multiply, n9001_c1_noise_44_run0 multiply
    "impulse": (8.051e-07, 2.724e-07),                  # n1000_c1_impulse_44_run1 multiply, n8192_c3_impulse_44_run0 multiply
    "step": (3.967e-05, 1.194e-04),                     # n9001_c3_step_44_run0 multiply (the restatement's own error there: 3.968e-5, 1.197e-4)
}
BOUNDS = {kind: (2.0 * rms, 2.0 * peak) for kind, (rms, peak) in MEASURED.items()}
# Audio::shift_frequency end to end (test_gpu_halfband's case: 2 x 9001 frames of noise, a shift swinging through +-300 Hz), by the same
# rule: twice what the MI355X measured against the fp32 restatement.  Nearly all of it is the two order-8 filters before the network: the
# fp32 restatement is itself 7.391e-6 and 2.988e-5 from the truth there (a high-pass at 30 Hz has g of 2e-3), the device 7.385e-6 and 3.687e-5
SHIFT_MEASURED = (8.881e-06, 3.991e-05)
SHIFT_BOUNDS = (2.0 * SHIFT_MEASURED[0], 2.0 * SHIFT_MEASURED[1])


def poles():
    """:1109-1150 with ( 20, 5, 22000 ): ( first, second ) float32 [10].  The reference returns ( p_b, p_a ): the FIRST output's cascade has
    the odd-indexed poles of the design"""
    f_l, f_u = F32(5), F32(22000)
    B = F64(f_u / f_l)
    k = np.sqrt(1.0 - 1.0 / (B * B))
    L = 0.5 * (1.0 - np.sqrt(k)) / (1.0 + np.sqrt(k))
    A_p = L + 2.0 * np.power(L, 5.0) + 15.0 * np.power(L, 9.0)
    A = np.exp(np.pi * np.pi / np.log(A_p))
    n = 20.0
    r = np.arange(1, 21)
    phi = np.pi / 4.0 / n * (2 * r - 1)
    A2, A6 = A * A, A * A * A * A * A * A
    phi_p = np.arctan((A2 - A6) * np.sin(4.0 * phi) / (1.0 + (A2 + A6) * np.cos(4.0 * phi)))
    p = (np.sqrt(B) * np.tan(phi - phi_p) * 2.0 * np.pi * F64(f_l)).astype(F32)
    return p[1::2].copy(), p[0::2].copy()


def coefficients(sr):
    """G float32 [2][10] of the two cascades: :57, :67-68 with the pole as w"""
    T_half = PI / F32(sr)
    g = (np.stack(poles()) * T_half).astype(F32)
    return (g / (F32(1) + g)).astype(F32)


def cascade_rows(x, G, dtype=F32):
    """rows x [rows][n] through their cascades G [rows][10] (fp32), frame by frame, the sections in order, states from 0.  In `dtype`
    throughout: fp32 is the reference's arithmetic, one rounding per operation; fp64 the truth from the same G"""
    x = np.asarray(x).astype(dtype)
    G = np.asarray(G, F32).astype(dtype)
    rows, n = x.shape
    s = np.zeros((K, rows), dtype)
    out = np.empty((rows, n), dtype)
    with np.errstate(all="ignore"):
        for f in range(n):
            v_in = x[:, f]
            for i in range(K):
                v = G[:, i] * (v_in - s[i])                                            # :69
                lp = v + s[i]                                                          # :70
                s[i] = lp + v                                                          # :71
                v_in = lp - (v_in - lp)                                                # :79: lp * 1 + ( x - lp ) * -1
            out[:, f] = v_in
    return out


def network(x, sr, dtype=F32):
    """hilbert_phase_diff_network: x [ch][n] -> ( first, second ) [ch][n] in `dtype`"""
    x = np.asarray(x)
    ch = x.shape[0]
    G = coefficients(sr)
    both = cascade_rows(np.concatenate([x, x]), np.repeat(G, ch, axis=0), dtype)
    return both[:ch], both[ch:]


def state_space(G):
    """one cascade (G [10], fp32) as s' = A s + b x, y = c s + d x in fp64: a section is s' = ( 1 - 2 G ) s + 2 G x and puts out
    2 ( 1 - G ) s + ( 2 G - 1 ) x, which is the next section's x.  A is lower triangular"""
    G = np.asarray(G, F32).astype(F64)
    A, b = np.zeros((K, K)), np.zeros(K)
    c, d = np.zeros(K), 1.0                                                            # the section's input as c s + d x
    for i in range(K):
        A[i] = 2.0 * G[i] * c
        A[i, i] += 1.0 - 2.0 * G[i]
        b[i] = 2.0 * G[i] * d
        c = (2.0 * G[i] - 1.0) * c
        c[i] += 2.0 * (1.0 - G[i])
        d = (2.0 * G[i] - 1.0) * d
    return A, b, c, d


def response(sr, hz):
    """the two cascades' frequency responses at hz [m], complex128 [2][m], from the sections' own recurrences"""
    G = coefficients(sr).astype(F64)
    zi = np.exp(-2j * np.pi * np.asarray(hz, F64) / sr)                                # z^-1
    H = np.ones((2, len(zi)), np.complex128)
    for i in range(K):
        g = G[:, i:i + 1]
        H *= (2.0 * g - 1.0) + 2.0 * (1.0 - g) * 2.0 * g * zi / (1.0 - (1.0 - 2.0 * g) * zi)
    return H


def cos_sin(phase):
    """std::exp( complex<float>( 0, phase ) ): the fp64 functions of the fp32 phase rounded to fp32 once"""
    p = np.asarray(phase, F32).astype(F64)
    return np.cos(p).astype(F32), np.sin(p).astype(F32)


def combine(first, second, re, im, dtype=F32):
    """:1179-1181, :1258: first * re - second * im, two products and a difference in `dtype`"""
    t = dtype
    with np.errstate(all="ignore"):
        a = (np.asarray(first).astype(t) * np.asarray(re).astype(t)).astype(t)
        b = (np.asarray(second).astype(t) * np.asarray(im).astype(t)).astype(t)
        return (a - b).astype(t)


def shift_curves(shift, sr, low_cutoff=30.0):
    """:1195-1219 from the sampled shift [n] (fp32), all in fp32: ( lp_curve, hp_curve, phase ).  The index round trip frame -> time -> frame
    is the identity at these lengths.  phase is the SEQUENTIAL exclusive sum of shift * pi2 / sr from 0.0f"""
    s = np.asarray(shift, F32)
    sr = F32(sr)
    high = sr / F32(2) - F32(1000)
    lp = np.where(s > 0, high - s, high).astype(F32)
    hp = np.where(s < 0, F32(low_cutoff) - s, F32(low_cutoff)).astype(F32)
    step = (s * PI2 / sr).astype(F32)
    phase = np.zeros(len(s), F32)
    if len(s) > 1:
        phase[1:] = np.cumsum(step[:-1], dtype=F32)                                    # one fp32 addition per frame, in order
    return lp, hp, phase


def shift_frequency(x, sr, shift, low_cutoff=30.0, dtype=F32):
    """Audio::shift_frequency with the shift sampled [n]: the order-8 low-pass and high-pass of filter_reference, then the network and
    the modulator exp( i phase ).  fp64: the truth from the same fp32 curves, phase, cos and sin, in fp64 between the stages as well"""
    lp, hp, phase = shift_curves(shift, sr, low_cutoff)
    y = R1.filter_1pole(x, sr, lp, R1.BUTTERWORTH_LOW, 8, dtype)
    g = R1.coefficients(hp, sr, y.shape[1])
    for poles_, R, tap in R1.sections(R1.BUTTERWORTH_HIGH, 8):                         # filter_reference.cascade, which would round y to fp32 first
        y = np.stack([R1.section_1pole(row, g, tap, dtype) if poles_ == 1 else R1.section_2pole(row, g, R, tap, dtype) for row in y])
    first, second = network(y, sr, dtype)
    return combine(first, second, *cos_sin(phase), dtype)


def scale(x):
    """( rms, peak ) of an input"""
    x = np.asarray(x, F64)
    return float(np.sqrt(np.mean(x * x))), float(np.max(np.abs(x)))


def errors(got, want, rms_x, peak_x):
    """( rms, max ) of got - want, divided by the rms and the peak of the INPUT (filter_reference.errors)"""
    d = np.asarray(got, F64) - np.asarray(want, F64)
    return float(np.sqrt(np.mean(d * d))) / rms_x, float(np.max(np.abs(d))) / peak_x


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def noise(ch, n, seed):
    """uniform noise of rms 0.3"""
    return (np.random.default_rng(seed).uniform(-1.0, 1.0, (ch, n)) * (0.3 * np.sqrt(3.0))).astype(F32)


def impulse(ch, n):
    x = np.zeros((ch, n), F32)
    for c in range(ch):
        x[c, min(c, n - 1)] = 1.0 / (c + 1)
    return x


def step(ch, n):
    x = np.zeros((ch, n), F32)
    for c in range(ch):
        x[c, min(2 * c, n - 1):] = 0.5 / (c + 1)
    return x


INPUTS = {"noise": noise, "impulse": lambda ch, n, seed: impulse(ch, n), "step": lambda ch, n, seed: step(ch, n)}


def rows_re_im(n, sr):
    """a complex modulator that is no unit phasor, sampled: ( re, im ) float32 [n]"""
    t = np.arange(n) / sr
    return (0.1 + 0.8 * np.cos(2 * np.pi * 300.0 * t)).astype(F32), (0.6 * np.sin(2 * np.pi * 170.0 * t + 0.3)).astype(F32)


def phase_row(n, sr):
    """the phase of a shift that swings between -400 and +400 Hz, summed in fp32 as shift_frequency does"""
    shift = (400.0 * np.sin(2 * np.pi * 7.0 * np.arange(n) / sr)).astype(F32)
    return shift_curves(shift, sr)[2]


def _case(n, ch, sr, kind, run):
    seed = 100 + n % 97 + 7 * ch
    b_ch, b_n, b_sr = (2, n + 5, 44100.0 if sr == 48000.0 else 48000.0)
    c = {"name": "n%d_c%d_%s_%d_run%d" % (n, ch, kind, int(sr) // 1000, run), "kind": kind, "x": INPUTS[kind](ch, n, seed), "sr": sr, "run": run,
         "b": noise(b_ch, b_n, seed + 1), "b_sr": b_sr}
    c["re"], c["im"] = rows_re_im(n, sr)
    c["phase"] = phase_row(n, sr)
    return c


# run 1: a block is 256 frames -- one frame, one quad short, a block less one, a block, a block and one, four blocks with a ragged tail;
# run 0 (the library's, 16): three blocks unaligned, two blocks of whole quads (the 16-byte loads and stores).  Channels 1 and 3, both
# sample rates and the three inputs in turn
CASES = [_case(*a) for a in (
    (1, 1, 48000.0, "noise", 1), (3, 3, 44100.0, "impulse", 1), (255, 3, 48000.0, "noise", 1), (256, 1, 44100.0, "step", 1),
    (257, 1, 44100.0, "noise", 1), (1000, 3, 48000.0, "noise", 1), (1000, 1, 44100.0, "impulse", 1), (1000, 3, 44100.0, "step", 1),
    (9001, 3, 48000.0, "noise", 0), (9001, 1, 44100.0, "noise", 0), (9001, 1, 48000.0, "impulse", 0), (9001, 3, 44100.0, "step", 0),
    (8192, 3, 48000.0, "noise", 0), (8192, 1, 44100.0, "step", 0), (8192, 3, 44100.0, "impulse", 0))]
IDS = [c["name"] for c in CASES]
RESULTS = ("first", "second", "rows", "phase", "multiply")


def case(name):
    return CASES[IDS.index(name)]


@functools.lru_cache(maxsize=None)
def expected(name, dtype=F32):
    """{ result: array } of a case in `dtype` from the sequential loops, computed once and shared: treat as read-only.  All five results
    come from two passes over the frames (the case's channels and the second operand's)"""
    c = case(name)
    first, second = network(c["x"], c["sr"], dtype)
    ch, n = min(c["x"].shape[0], c["b"].shape[0]), min(c["x"].shape[1], c["b"].shape[1])
    b_x, b_y = network(c["b"][:ch, :n], c["b_sr"], dtype)
    out = {"first": first, "second": second, "rows": combine(first, second, c["re"], c["im"], dtype),
           "phase": combine(first, second, *cos_sin(c["phase"]), dtype), "multiply": combine(first[:ch, :n], second[:ch, :n], b_x, b_y, dtype)}
    for v in out.values():
        v.setflags(write=False)
    return out


def scales(c):
    """{ result: ( rms, peak ) } the errors of a case's results are divided by"""
    rms, peak = scale(c["x"])
    ch, n = min(c["x"].shape[0], c["b"].shape[0]), min(c["x"].shape[1], c["b"].shape[1])
    rms_a, peak_a = scale(c["x"][:ch, :n])
    rms_b, peak_b = scale(c["b"][:ch, :n])
    out = {r: (rms, peak) for r in RESULTS}
    out["multiply"] = (rms_a * rms_b, peak_a * peak_b)
    return out
