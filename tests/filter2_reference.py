"""Audio::filter_2pole_lowpass / _bandpass / _highpass / _notch (Audio/AudioFilter.cpp:520-624), filter_2pole_lowshelf / _bandshelf /
_highshelf (:631-758) and filter_1pole_lowshelf / _highshelf (:431-512) restated in NumPy.  DESIGN.md 4.16.

    sections()               the cascade of a kind and order as a list of ( poles, out, role, pole )
    section_rows()           the per-frame part of one section: g, R and m [n] in fp32, from the cutoff, the damping and the gain
    loop_section()           the sequential loop (:61-74, :164-182) with the frame's own g and R in fp32, one rounding per operation, or in
                             fp64 from the SAME fp32 g, R and m (the "truth": same coefficients, exact recurrence and mix)
    scan_section( run )      the model of the device: per section the state at every run's first frame from an fp64 recurrence over the
                             section's affine maps (built from the fp32 step values), rounded to fp32 once, then the fp32 loop over the run
    filter2()                all of it
    errors(), CASES with their two classes
    LONG, long_case()        rows of more than 256 blocks, past one pass of the carry kernel (the windows are filter_reference's)

Every transcendental (acos, cos, sin, sqrt, pow, hypot, tan) is the fp64 function of the fp32 argument rounded to fp32 once, complex
products and quotients are the textbook forms with one rounding per operation: what the device kernels do."""
import functools

import numpy as np

import filter_reference as R1

F32, F64 = np.float32, np.float64
RUN, WAVE, BLOCK = R1.RUN, R1.WAVE, R1.BLOCK
SHELF1_LOW, SHELF1_HIGH, LOW, BAND, HIGH, NOTCH, LOWSHELF, BANDSHELF, HIGHSHELF = range(9)          # FLANHIP_FILTER2_*
KIND_NAMES = ("shelf1low", "shelf1high", "low", "band", "high", "notch", "lowshelf", "bandshelf", "highshelf")
# a section's output: the taps, then the mixes of ( lp, b = bp * 2 * R, hp ) with the frame's m
TAP_LOW, TAP_HIGH, TAP_BAND, MIX_TILT1, MIX_TILT2, MIX_LOWSHELF, MIX_HIGHSHELF, MIX_BANDSHELF = range(8)
OUTPUTS = (MIX_TILT2, MIX_TILT2, TAP_LOW, TAP_BAND, TAP_HIGH, TAP_BAND, MIX_LOWSHELF, MIX_BANDSHELF, MIX_HIGHSHELF)
# which section of the cascade: the tilt's 1-pole section and its 2-pole sections; the 2-pole families' real pole, pole w scaler, pole w / scaler
TILT_1POLE, TILT_2POLE, REAL_POLE, POLE_TIMES, POLE_OVER = range(5)
PI, PI2 = R1.PI, R1.PI2
errors = R1.errors
# What the device (and the scan model) is held to.  Against the fp32 restatement, parity cases: rms( got - want ) / rms( x ) and
# max | got - want | / max | x |.  The scan model on the CPU gives at most 3.409e-7 (highshelf4_1k_d025_p6) and 2.146e-6
# (n4096_highshelf3_all) at the default run; the MI355X measures the same 3.409e-7 and 2.146e-6 on the same two cases.  The bounds are
# at most 30 % above
REL_RMS_BOUND = 4.4e-7
REL_MAX_BOUND = 2.7e-6
# against the fp64 truth, both classes: at most 4 x the restatement's own error on the same case, or 8 fp32 ulps of the input's scale
TRUTH_FACTOR = 4.0
TRUTH_FLOOR = 8 * 2.0 ** -23


def _f64fn(fn, *args):
    """the fp64 function of fp32 arguments, rounded to fp32 once"""
    with np.errstate(all="ignore"):
        return fn(*(np.asarray(a, F32).astype(F64) for a in args)).astype(F32)


def amp(decibel):
    """defines.h: pow( 10.0f, d / 20.0f )"""
    return _f64fn(lambda d: np.power(10.0, d), np.asarray(decibel, F32) / F32(20))


def poles(order):
    """:32-44: the Butterworth poles above the axis, ( cos theta_i, sin theta_i ) in fp32"""
    out = []
    for i in range(order // 2):
        delta = PI2 / F32(order * 2)
        theta = delta * F32(i) + PI / F32(2) + delta / F32(2)
        out.append((F32(np.cos(F64(theta))), F32(np.sin(F64(theta)))))
    return out


def sections(kind, order):
    """[( poles, out, role, ( pre, pim ) )].  The tilt: for odd N a 1-pole section FIRST, then a 2-pole section per pole.  The 2-pole
    families: for odd N the real pole's section FIRST, then per pole TWO sections: order N is N state-variable sections"""
    tilt = kind in (SHELF1_LOW, SHELF1_HIGH)
    zero = (F32(0), F32(0))
    out = []
    if order % 2:
        out.append((1, MIX_TILT1, TILT_1POLE, zero) if tilt else (2, OUTPUTS[kind], REAL_POLE, zero))
    for p in poles(order):
        if tilt:
            out.append((2, OUTPUTS[kind], TILT_2POLE, p))
        else:
            out += [(2, OUTPUTS[kind], POLE_TIMES, p), (2, OUTPUTS[kind], POLE_OVER, p)]
    return out


def clamp(cutoff, sr):
    """std::clamp( c, 1, sr / 2 ) by two comparisons: a NaN stays"""
    nyquist = F32(sr) / F32(2)
    c = np.asarray(cutoff, F32)
    with np.errstate(all="ignore"):
        return np.where(c < F32(1), F32(1), np.where(nyquist < c, nyquist, c)).astype(F32)


def g_of(w, sr):
    """:29, :67 / :170: every section prewarps its own cutoff, no clamp"""
    T_half = PI / F32(sr)
    with np.errstate(all="ignore"):
        return ((_f64fn(np.tan, T_half * w) / T_half) * T_half).astype(F32)


def section_rows(kind, order, role, pole, cutoff, damping, gain, sr, n):
    """( g, R, m ) [n] in fp32 of one section; cutoff, damping, gain: scalars or [n]"""
    c, D, G = (np.broadcast_to(np.asarray(v, F32), (n,)) for v in (cutoff, damping, gain))
    two_n, N = F32(2 * order), F32(order)
    pre, pim = pole
    with np.errstate(all="ignore"):
        if kind in (SHELF1_LOW, SHELF1_HIGH):
            M = amp((-G if kind == SHELF1_HIGH else G) / two_n)                        # :466, :509
            w = M * clamp(c, sr)                                                       # :453, :468
            if role == TILT_1POLE:
                return g_of(w, sr), np.zeros(n, F32), M
            return g_of(w, sr), (pre / w).astype(F32), (M * M).astype(F32)             # :479, :467
        if kind <= NOTCH:
            w, R, M = clamp(c, sr), D, np.ones(n, F32)                                 # :534-535
        else:
            band = kind == BANDSHELF
            M = amp((-G if band else G / F32(2)) / two_n)                              # :647, :720, :737, :754
            w = c if band else (c * M).astype(F32)                                     # no clamp
            R = (D * M).astype(F32) if band else D
        alpha = (_f64fn(np.arccos, R) / N).astype(F32)                                 # :547
        if role == REAL_POLE:
            wk, Rk = w, _f64fn(np.cos, alpha)                                          # :553
        else:
            real = R > F32(1)                                                          # :561-563
            root = _f64fn(np.sqrt, R * R - F32(1))
            sc_re = np.where(real, _f64fn(np.power, R + root, np.broadcast_to(F32(1) / N, (n,))), _f64fn(np.cos, -alpha)).astype(F32)
            sc_im = np.where(real, F32(0), _f64fn(np.sin, -alpha)).astype(F32)
            a, b = (pre * w).astype(F32), (pim * w).astype(F32)                        # :565
            if role == POLE_TIMES:
                re, im = a * sc_re - b * sc_im, a * sc_im + b * sc_re                  # :568
            else:
                den = sc_re * sc_re + sc_im * sc_im
                re, im = (a * sc_re + b * sc_im) / den, (b * sc_re - a * sc_im) / den  # :573
            wk = _f64fn(np.hypot, re, im)                                              # :569
            Rk = (-re / wk).astype(F32)                                                # :570
        return g_of(wk, sr), np.asarray(Rk, F32), (M * M).astype(F32)


def step_values(g, R, poles_, dtype=F32):
    """what a step needs of g and R, per frame, in `dtype` from the fp32 rows: ( G, ) or ( g, g1, d )"""
    g, R, t = np.asarray(g, F32).astype(dtype), np.asarray(R, F32).astype(dtype), dtype
    with np.errstate(all="ignore"):
        if poles_ == 1:
            return (g / (t(1) + g),)                                                   # :68
        return g, t(2) * R + g, t(1) / (t(1) + t(2) * R * g + g * g)                   # :171-172


def mix(out, x, lp, bp, hp, R, m, dtype=F32):
    """a section's output from its three (a 1-pole section: lp alone), per frame and stateless: the reference's operations in its order"""
    t = dtype
    R, m = np.asarray(R, F32).astype(t), np.asarray(m, F32).astype(t)
    with np.errstate(all="ignore"):
        if out == MIX_TILT1:
            return lp * m + (x - lp) / m                                               # :474
        if out == TAP_LOW:
            return lp
        if out == TAP_HIGH:
            return hp
        b = bp * t(2) * R                                                              # :181
        if out == TAP_BAND:
            return b
        if out == MIX_TILT2:
            return lp / m + b + hp * m                                                 # :482
        if out == MIX_LOWSHELF:
            return lp / (m * m) + b / m + hp                                           # :721
        if out == MIX_HIGHSHELF:
            return lp + b * m + hp * m * m                                             # :755
        assert out == MIX_BANDSHELF
        return lp + b / m + hp                                                         # :738


def _items(a, dtype):
    return a.tolist() if dtype == F64 else list(a)


def _loop(x, vals, poles_, dtype, s1, s2):
    """the section's recurrence over x [n] from ( s1, s2 ): ( lp, bp, hp ) [n] in `dtype`"""
    n = len(x)
    xs = _items(np.asarray(x).astype(dtype), dtype)
    lp_, bp_, hp_ = np.zeros(n, dtype), np.zeros(n, dtype), np.zeros(n, dtype)
    with np.errstate(all="ignore"):
        if poles_ == 1:
            Gs = _items(vals[0], dtype)
            for f in range(n):
                v = Gs[f] * (xs[f] - s1)
                lp = v + s1
                s1 = lp + v
                lp_[f] = lp
        else:
            gs, g1s, ds = (_items(v, dtype) for v in vals)
            for f in range(n):
                hp = (xs[f] - g1s[f] * s1 - s2) * ds[f]
                v1 = gs[f] * hp
                bp = v1 + s1
                s1 = bp + v1
                v2 = gs[f] * bp
                lp = v2 + s2
                s2 = lp + v2
                lp_[f], bp_[f], hp_[f] = lp, bp, hp
    return lp_, bp_, hp_


def loop_section(x, g, R, m, poles_, out, dtype=F32):
    """one section over one channel x [n], states from 0"""
    zero = 0.0 if dtype == F64 else F32(0)
    xd = np.asarray(x).astype(dtype)
    lp, bp, hp = _loop(xd, step_values(g, R, poles_, dtype), poles_, dtype, zero, zero)
    return mix(out, xd, lp, bp, hp, R, m, dtype)


def scan_section(x, g, R, m, poles_, out, run):
    """one section over one channel as the device runs it: every run replayed in fp32 from its fp64 start state rounded once"""
    n = len(x)
    vals = step_values(g, R, poles_, F32)
    with np.errstate(all="ignore"):
        start = np.asarray(R1._run_start_states(x, vals, poles_, run), F64).astype(F32)      # [runs][2]
    runs = start.shape[0]

    def grid(v):
        padded = np.zeros(runs * run, F32)
        padded[:n] = v
        return padded.reshape(runs, run)
    xg = grid(x)
    lp_, bp_, hp_ = np.zeros((runs, run), F32), np.zeros((runs, run), F32), np.zeros((runs, run), F32)
    s1, s2 = start[:, 0].copy(), start[:, 1].copy()
    with np.errstate(all="ignore"):
        if poles_ == 1:
            G = grid(vals[0])
            for i in range(run):
                v = G[:, i] * (xg[:, i] - s1)
                lp = v + s1
                s1 = lp + v
                lp_[:, i] = lp
        else:
            gg, g1, d = (grid(v) for v in vals)
            for i in range(run):
                hp = (xg[:, i] - g1[:, i] * s1 - s2) * d[:, i]
                v1 = gg[:, i] * hp
                bp = v1 + s1
                s1 = bp + v1
                v2 = gg[:, i] * bp
                lp = v2 + s2
                s2 = lp + v2
                lp_[:, i], bp_[:, i], hp_[:, i] = lp, bp, hp
    flat = [v.reshape(-1)[:n] for v in (lp_, bp_, hp_)]
    return mix(out, np.asarray(x, F32), flat[0], flat[1], flat[2], R, m, F32)


def filter2(x, sr, cutoff, damping, gain, kind, order, dtype=F32, run=None):
    """the whole call, [ch][n] -> [ch][n] in `dtype`; run: the scan model at that run length instead of the sequential loop (fp32)"""
    x = np.asarray(x, F32)
    n = x.shape[1]
    y = x.astype(dtype)
    for poles_, out, role, pole in sections(kind, order):
        g, R, m = section_rows(kind, order, role, pole, cutoff, damping, gain, sr, n)
        if run is not None:
            y = np.stack([scan_section(row, g, R, m, poles_, out, run) for row in y])
        else:
            y = np.stack([loop_section(row, g, R, m, poles_, out, dtype) for row in y])
    t = dtype
    with np.errstate(all="ignore"):
        if kind == NOTCH:                                                              # :621-623; order 0: the band-pass is a copy
            y = (t(0) + (-y)) + x.astype(t)
        if kind in (SHELF1_LOW, SHELF1_HIGH):                                          # :498, :510
            y = y * np.broadcast_to(amp(np.asarray(gain, F32) / F32(2)), (n,)).astype(t)
    return y.astype(dtype)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SR = R1.SR
N3 = R1.N3
LENGTHS = R1.LENGTHS
POISON_FRAME = 5000
noise, sine, sweep, wobble = R1.noise, R1.sine, R1.sweep, R1.wobble


def damping_curve(n, lo, hi, hz=3.0):
    """the damping swinging between lo and hi"""
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return (mid + half * np.sin(2 * np.pi * hz * np.arange(n) / SR)).astype(F32)


def gain_curve(n):
    """+-12 dB, two and a half swings over 12 305 frames"""
    return (12.0 * np.sin(2 * np.pi * 10.0 * np.arange(n) / SR)).astype(F32)


CUTOFFS = {"1k": lambda n: 1000.0, "sweep": sweep, "wobble": wobble}
# dampings: a scalar, a curve inside [0.1, 0.9], and -- with even orders only -- one through [0.1, 1.5]
DAMPINGS = {"d07": lambda n: 0.70710677, "d025": lambda n: 0.25, "dcurve": lambda n: damping_curve(n, 0.1, 0.9), "dover": lambda n: damping_curve(n, 0.1, 1.5)}
GAINS = {"p6": lambda n: 6.0, "m12": lambda n: -12.0, "gcurve": gain_curve}
PARITY, TRUTH_ONLY = "parity", "truth_only"
# the cases held to the truth criterion alone, by name: the damping 0.02 resonances (the fp32 loop itself is 4e-6 ... 7e-6 from the truth
# there) and the 1-pole shelves at orders 2 and 3, where the reference is unstable (R negative) and its fp32 loop 1e-5 ... 4e-4 from the truth
TRUTH_ONLY_NAMES = ("low2_res002", "band3_res002", "high4_res002", "shelf1low2", "shelf1low3", "shelf1high2", "shelf1high3")


def _case(name, x, cutoff, damping, gain, kind, order, cls=PARITY):
    assert x.shape[0] <= 3 and x.shape[1] <= N3
    if name in TRUTH_ONLY_NAMES:
        cls = TRUTH_ONLY
    return {"name": name, "x": x, "sr": SR, "cutoff": cutoff, "damping": damping, "gain": gain, "kind": kind, "order": order, "cls": cls}


def _make_cases():
    cases = []
    # every kind at orders 0 ... 4 (the 1-pole shelves 0 ... 3: at order 4 the reference's own fp32 loop is 1e-2 from the truth, outputs
    # x 1e3) over three blocks and a ragged tail; the cutoffs, dampings, gains and channel counts in turn.  Scalar, mixed and all-curve
    # arguments all occur: 1k / d07 / d025 / p6 / m12 are scalars.  A damping that passes 1 goes with even orders only
    i = 0
    for kind in range(9):
        for order in range(5):
            if kind <= SHELF1_HIGH and order == 4:
                continue
            cut = ("1k", "sweep", "wobble")[i % 3]
            damp = ("d07", "dcurve", "d025", "dover")[i % 4]
            if damp == "dover" and order % 2:
                damp = "dcurve"
            gn = ("p6", "gcurve", "m12")[(i // 2) % 3]
            if kind == BANDSHELF and order % 2:
                gn = "p6"                                  # R = damping * M with M < 1: a negative gain would take it past 1
            if kind <= SHELF1_HIGH and order >= 2:
                name, gn = "%s%d" % (KIND_NAMES[kind], order), ("p6" if kind == SHELF1_LOW else "m12")
            else:
                name = "%s%d_%s_%s_%s" % (KIND_NAMES[kind], order, cut, damp, gn)
            cases.append(_case(name, noise(1 + i % 3, N3, 700 + i), CUTOFFS[cut](N3), DAMPINGS[damp](N3), GAINS[gn](N3), kind, order))
            i += 1
    # every length of filter.hip's table
    by_length = ((LOW, 3), (HIGHSHELF, 4), (BAND, 2), (SHELF1_LOW, 1), (NOTCH, 3), (BANDSHELF, 2), (LOWSHELF, 3), (HIGH, 4), (SHELF1_HIGH, 1))
    for j, n in enumerate(LENGTHS):
        kind, order = by_length[j]
        damp = "dover" if order % 2 == 0 else "dcurve"
        cases.append(_case("n%d_%s%d" % (n, KIND_NAMES[kind], order), noise(1 + j % 3, n, 800 + j), sweep(n), DAMPINGS[damp](n), gain_curve(n), kind, order))
    # lengths that are multiples of 4, one block exactly and three with a tail of whole quads, 2 and 3 channels: the 16-byte loads and stores
    quads = ((BLOCK, 2, LOW, 4, "all"), (BLOCK, 3, HIGHSHELF, 3, "all"), (BLOCK, 2, SHELF1_HIGH, 1, "all"), (N3 - 1, 3, NOTCH, 2, "mixed"),
             (N3 - 1, 2, BANDSHELF, 4, "all"), (N3 - 1, 2, BAND, 3, "scalar"), (N3 - 1, 3, LOWSHELF, 2, "mixed"), (N3 - 1, 2, HIGH, 1, "all"))
    for j, (n, ch, kind, order, form) in enumerate(quads):
        assert n % 4 == 0
        damp = DAMPINGS["dover" if order % 2 == 0 else "dcurve"](n) if form == "all" else 0.3
        cutoff = 1000.0 if form == "scalar" else wobble(n)
        gain = gain_curve(n) if form == "all" else -12.0
        cases.append(_case("n%d_%s%d_%s" % (n, KIND_NAMES[kind], order, form), noise(ch, n, 900 + j), cutoff, damp, gain, kind, order))
    # the resonances: damping 0.02 is a peak of 25 at the cutoff
    cases.append(_case("low2_res002", noise(2, N3, 21), 1000.0, 0.02, 0.0, LOW, 2))
    cases.append(_case("band3_res002", noise(1, N3, 22), sweep(N3), 0.02, 0.0, BAND, 3))
    cases.append(_case("high4_res002", noise(2, N3, 23), wobble(N3), 0.02, 0.0, HIGH, 4))
    # a NaN cutoff at one frame, and a damping above 1 at one frame on an odd order (alpha = acos( R ) / N is NaN there), with their clean twins
    curve = sweep(N3)
    cases.append(_case("clean_low3", noise(2, N3, 8), curve, 0.5, 0.0, LOW, 3))
    poisoned = curve.copy()
    poisoned[POISON_FRAME] = np.nan
    cases.append(_case("nan_low3", noise(2, N3, 8), poisoned, 0.5, 0.0, LOW, 3, cls=None))
    damp = damping_curve(N3, 0.2, 0.8)
    cases.append(_case("clean_highshelf3", noise(2, N3, 9), 2000.0, damp, 6.0, HIGHSHELF, 3))
    over = damp.copy()
    over[POISON_FRAME] = 1.25
    cases.append(_case("over1_highshelf3", noise(2, N3, 9), 2000.0, over, 6.0, HIGHSHELF, 3, cls=None))
    return cases


CASES = _make_cases()
IDS = [c["name"] for c in CASES]
PARITY_IDS = [c["name"] for c in CASES if c["cls"] == PARITY]
TRUTH_ONLY_IDS = [c["name"] for c in CASES if c["cls"] == TRUTH_ONLY]
CHECKED_IDS = PARITY_IDS + TRUTH_ONLY_IDS
assert len(set(IDS)) == len(IDS)
assert sorted(TRUTH_ONLY_IDS) == sorted(TRUTH_ONLY_NAMES)


def case(name):
    return CASES[IDS.index(name)]


def call(c, dtype=F32, run=None, x=None):
    return filter2(c["x"] if x is None else x, c["sr"], c["cutoff"], c["damping"], c["gain"], c["kind"], c["order"], dtype, run)


@functools.lru_cache(maxsize=None)
def expected(name, dtype=F32):
    """the sequential loop's output of a case in `dtype`, computed once and shared: treat as read-only"""
    out = call(case(name), dtype)
    out.setflags(write=False)
    return out


# ---- rows longer than one pass of the carry kernel (filter_reference.py has the geometry) --------------------------------------------
PASS_RUNS, LONG_RUN1, N_THREE_PASSES, N_LONG = R1.PASS_RUNS, R1.LONG_RUN1, R1.N_THREE_PASSES, R1.N_LONG
windows, errors_over, figures = R1.windows, R1.errors_over, R1.figures
MEMORY_CUTOFF, memory_inputs = R1.MEMORY_CUTOFF, R1.memory_inputs
# A window of fewer frames than a block has no rms to speak of: the second pass of 65 537 frames is ONE frame, 3 samples, and their rms
# is a maximum in all but name (the high shelf puts out 1.9 for a peak of 1 there).  Such a window's rms has a constant of its own:
# measured on the MI355X 1.341e-6 (highshelf3_dcurve_p6_n65537_run1, pass 1), and the scan model on the CPU gives the same 1.341e-6;
# at most 30 % above.  Its maximum, and both figures of every longer window, are held to REL_RMS_BOUND / REL_MAX_BOUND as they stand
SHORT_WINDOW_REL_RMS_BOUND = 1.7e-6


def rms_bound(lo, hi):
    return REL_RMS_BOUND if hi - lo >= 256 else SHORT_WINDOW_REL_RMS_BOUND


def _long_table():
    """noise under the swept cutoff.  low2_d025: the damping and the gain are scalars, the cutoff alone is a row; highshelf3_dcurve_p6: a
    damping row as well and a mix that reads the row m"""
    table = {}
    for i, n in enumerate(LONG_RUN1):
        table["low2_d025_n%d_run1" % n] = (LOW, 2, "d025", 0.0, 3, n, 1, 1100 + i)
        table["highshelf3_dcurve_p6_n%d_run1" % n] = (HIGHSHELF, 3, "dcurve", 6.0, 3, n, 1, 1110 + i)
    table["low2_d025_n%d" % N_LONG] = (LOW, 2, "d025", 0.0, 2, N_LONG, None, 1120)
    return table


LONG = _long_table()
LONG_IDS = list(LONG)


@functools.lru_cache(maxsize=None)
def long_case(name):
    """run: the forced run the row is meant for (None: the library's choice).  Built once: read-only"""
    kind, order, damp, gain, ch, n, run, seed = LONG[name]
    x, cutoff, damping = noise(ch, n, seed), sweep(n), DAMPINGS[damp](n)
    for v in (x, cutoff, damping):
        if not np.isscalar(v):
            v.setflags(write=False)
    return {"name": name, "x": x, "sr": SR, "cutoff": cutoff, "damping": damping, "gain": gain, "kind": kind, "order": order, "cls": PARITY, "run": run}


@functools.lru_cache(maxsize=None)
def long_expected(name, dtype=F32):
    """the sequential loop's output of a long case in `dtype`, computed once and shared: read-only"""
    out = call(long_case(name), dtype)
    out.setflags(write=False)
    return out
