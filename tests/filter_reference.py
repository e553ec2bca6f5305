"""Audio::filter_1pole_lowpass / _highpass (Audio/AudioFilter.cpp:327-387) and filter_1pole_repeat_low / _high (:280-324) restated in
NumPy.  DESIGN.md 4.15.

    coefficients()           the per-frame part (:19-30, :57, :67, :120): g [n] in fp32, shared by all channels and sections
    butterworth_R()          the dampings of the 2-pole sections (:32-44, :361), in fp32
    sections()               the cascade of a kind and order as a list of ( poles, R, tap )
    section_1pole / section_2pole / cascade
                             the sequential loop (:61-74, :164-182) in fp32, one rounding per operation, or in fp64 from the SAME fp32 g
                             and R (the "truth": same coefficients, exact recurrence)
    cascade_scan( run )      the model of the device: per section the state at every run's first frame from an fp64 recurrence over the
                             section's affine maps (built from the fp32 step values), rounded to fp32 once, then the fp32 loop over the run
    filter_1pole()           all of it
    errors(), CASES, stalls()
    LONG, long_case(), windows(), figures()
                             rows of more than 256 blocks, past one pass of the carry kernel, and the windows they are held over

tan (and the cosine of R) is the fp64 function of the fp32 argument rounded to fp32 once: what the device kernels do."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
RUN, WAVE, BLOCK = 16, 16 * 64, 16 * 256               # frames per lane, per wavefront, per block of filter.hip's scan
BUTTERWORTH_LOW, BUTTERWORTH_HIGH, REPEAT_LOW, REPEAT_HIGH = 0, 1, 2, 3      # FLANHIP_FILTER_*
LOW, HIGH = 0, 1                                       # a section's tap
PI = np.arccos(F32(-1))                                # defines.h:44: acosf( -1 ), a float
PI2 = PI * F32(2)
assert PI.dtype == F32


def coefficients(cutoff, sr, n):
    """g [n] in fp32.  cutoff: a scalar or [n].  std::clamp is two comparisons: a NaN cutoff stays NaN"""
    sr = F32(sr)
    T_half = PI / sr                                                                   # :57
    nyquist = sr / F32(2)
    c = np.broadcast_to(np.asarray(cutoff, F32), (n,))
    with np.errstate(all="ignore"):
        c = np.where(c < F32(1), F32(1), np.where(nyquist < c, nyquist, c)).astype(F32)    # :120
        w = np.tan((T_half * c).astype(F64)).astype(F32) / T_half                      # :29
        return (w * T_half).astype(F32)                                                # :67


def butterworth_R(order):
    """:32-44 and :361: R_i = -Re( exp( i theta_i ) ) for the floor( N / 2 ) poles above the axis"""
    out = []
    for i in range(order // 2):
        delta = PI2 / F32(order * 2)
        theta = delta * F32(i) + PI / F32(2) + delta / F32(2)
        out.append(-F32(np.cos(F64(theta))))
    return out


def sections(kind, order):
    """[( poles, R, tap )]: Butterworth: for odd N a 1-pole section FIRST, then the 2-pole sections; repeat: `order` 1-pole sections"""
    tap = HIGH if kind in (BUTTERWORTH_HIGH, REPEAT_HIGH) else LOW
    if kind in (REPEAT_LOW, REPEAT_HIGH):
        return [(1, F32(0), tap)] * order
    return ([(1, F32(0), tap)] if order % 2 else []) + [(2, R, tap) for R in butterworth_R(order)]


def step_values(g, poles, R, dtype=F32):
    """what a step needs of g, per frame, in `dtype` from the fp32 g and R: ( G, ) or ( g, g1, d )"""
    g = np.asarray(g, F32).astype(dtype)
    t = dtype
    with np.errstate(all="ignore"):
        if poles == 1:
            return (g / (t(1) + g),)                                                   # :68
        R = t(F32(R))
        return g, t(2) * R + g, t(1) / (t(1) + t(2) * R * g + g * g)                   # :171-172


def _items(a, dtype):
    """what the sequential loops iterate over: Python floats in fp64 (their arithmetic IS fp64), np.float32 scalars in fp32"""
    return a.tolist() if dtype == F64 else list(a)


def section_1pole(x, g, tap, dtype=F32):
    """:61-74 over one channel x [n], state from 0"""
    (G,) = step_values(g, 1, 0, dtype)
    xs, Gs = _items(np.asarray(x).astype(dtype), dtype), _items(G, dtype)
    s = 0.0 if dtype == F64 else F32(0)
    out = np.empty(len(xs), dtype)
    with np.errstate(all="ignore"):
        for f in range(len(xs)):
            v = Gs[f] * (xs[f] - s)
            lp = v + s
            s = lp + v
            out[f] = xs[f] - lp if tap else lp
    return out


def section_2pole(x, g, R, tap, dtype=F32):
    """:164-182 over one channel x [n], states from 0"""
    g_, g1, d = step_values(g, 2, R, dtype)
    xs, gs, g1s, ds = _items(np.asarray(x).astype(dtype), dtype), _items(g_, dtype), _items(g1, dtype), _items(d, dtype)
    s1 = s2 = 0.0 if dtype == F64 else F32(0)
    out = np.empty(len(xs), dtype)
    with np.errstate(all="ignore"):
        for f in range(len(xs)):
            hp = (xs[f] - g1s[f] * s1 - s2) * ds[f]
            v1 = gs[f] * hp
            bp = v1 + s1
            s1 = bp + v1
            v2 = gs[f] * bp
            lp = v2 + s2
            s2 = lp + v2
            out[f] = hp if tap else lp
    return out


def cascade(x, g, secs, dtype=F32):
    """x [ch][n] through the sections in turn: section k reads section k - 1's output, in `dtype` throughout"""
    y = np.asarray(x, F32).astype(dtype)
    for poles, R, tap in secs:
        y = np.stack([section_1pole(row, g, tap, dtype) if poles == 1 else section_2pole(row, g, R, tap, dtype) for row in y])
    return y


# ---- the scan form ------------------------------------------------------------------------------------------------------------------
def _run_start_states(x, vals, poles, run):
    """fp64 states before the first frame of every run of one channel: the section's affine maps, built from the fp32 step values
    converted to fp64, applied in frame order from the state 0"""
    n = len(x)
    xs = np.asarray(x, F64).tolist()
    starts = range(0, n, run)
    if poles == 1:
        G2 = (2.0 * vals[0].astype(F64))
        a, b = (1.0 - G2).tolist(), G2.tolist()
        s, out = 0.0, []
        for f in range(n):
            if f % run == 0:
                out.append((s, 0.0))
            s = a[f] * s + b[f] * xs[f]
        return out
    g, g1, d = (v.astype(F64) for v in vals)
    gd = g * d
    ggd = g * gd
    a11, a12, a21, a22 = (1.0 - 2.0 * gd * g1).tolist(), (-2.0 * gd).tolist(), (2.0 * g * (1.0 - gd * g1)).tolist(), (1.0 - 2.0 * ggd).tolist()
    b1, b2 = (2.0 * gd).tolist(), (2.0 * ggd).tolist()
    s1 = s2 = 0.0
    out = []
    for f in range(n):
        if f % run == 0:
            out.append((s1, s2))
        s1, s2 = a11[f] * s1 + a12[f] * s2 + b1[f] * xs[f], a21[f] * s1 + a22[f] * s2 + b2[f] * xs[f]
    assert len(out) == len(starts)
    return out


def _section_scan(x, g, poles, R, tap, run):
    """one section over one channel as the device runs it: every run replayed in fp32 from its fp64 start state rounded once.  The runs
    are independent then, so the replay goes over all of them at once"""
    n = len(x)
    vals = step_values(g, poles, R, F32)
    with np.errstate(all="ignore"):
        start = np.asarray(_run_start_states(x, vals, poles, run), F64).astype(F32)       # [runs][2]
    runs = start.shape[0]

    def grid(v):
        padded = np.zeros(runs * run, F32)
        padded[:n] = v
        return padded.reshape(runs, run)
    xg = grid(x)
    out = np.empty((runs, run), F32)
    s1, s2 = start[:, 0].copy(), start[:, 1].copy()
    with np.errstate(all="ignore"):
        if poles == 1:
            G = grid(vals[0])
            for i in range(run):
                v = G[:, i] * (xg[:, i] - s1)
                lp = v + s1
                s1 = lp + v
                out[:, i] = xg[:, i] - lp if tap else lp
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
                out[:, i] = hp if tap else lp
    return out.reshape(-1)[:n]


def cascade_scan(x, g, secs, run=RUN):
    """the model of the device: fp32 [ch][n]"""
    y = np.asarray(x, F32)
    for poles, R, tap in secs:
        y = np.stack([_section_scan(row, g, poles, R, tap, run) for row in y])
    return y


def filter_1pole(x, sr, cutoff, kind, order, dtype=F32, run=None):
    """the whole call, [ch][n] -> [ch][n] in `dtype`; run: the scan model at that run length instead of the sequential loop (fp32).
    Order 0: Butterworth copies (:337), repeat leaves its zero-initialised output (:289, :299)"""
    x = np.asarray(x, F32)
    if order == 0:
        return x.astype(dtype) if kind in (BUTTERWORTH_LOW, BUTTERWORTH_HIGH) else np.zeros(x.shape, dtype)
    g = coefficients(cutoff, sr, x.shape[1])
    if run is not None:
        return cascade_scan(x, g, sections(kind, order), run)
    return cascade(x, g, sections(kind, order), dtype)


def errors(got, want, x):
    """( rms, max ) of got - want, divided by the rms and the peak of the INPUT x: a filter's rounding scales with what passes through
    its states, not with what comes out (an order-8 high-pass of a 440 Hz tone puts out a tenth of it)"""
    got, want, x = np.asarray(got, F64), np.asarray(want, F64), np.asarray(x, F64)
    d = got - want
    rms_x, peak_x = float(np.sqrt(np.mean(x * x))), float(np.max(np.abs(x)))
    if peak_x == 0.0:
        return (0.0, 0.0) if not np.any(d) else (np.inf, np.inf)
    return float(np.sqrt(np.mean(d * d))) / rms_x, float(np.max(np.abs(d))) / peak_x


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SR = 48000.0
LENGTHS = (1, RUN - 1, RUN, RUN + 1, WAVE - 1, WAVE + 1, BLOCK - 1, BLOCK + 1, 3 * BLOCK + 17)
N3 = 3 * BLOCK + 17                                    # 12 305: three blocks and a ragged tail
NAN_FRAME = 5000
KIND_NAMES = {BUTTERWORTH_LOW: "low", BUTTERWORTH_HIGH: "high", REPEAT_LOW: "rlow", REPEAT_HIGH: "rhigh"}


def noise(ch, n, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (ch, n)).astype(F32)


def sine(ch, n, hz=440.0):
    t = np.arange(n) / SR
    return np.stack([(0.8 / (c + 1)) * np.sin(2 * np.pi * hz * t + c) for c in range(ch)]).astype(F32)


def sweep(n):
    """200 -> 8000 Hz, exponential"""
    return (200.0 * (8000.0 / 200.0) ** (np.arange(n) / max(n - 1, 1))).astype(F32)


def wobble(n):
    """the cutoff swinging between 100 and 3900 Hz fifty times a second"""
    return (2000.0 + 1900.0 * np.sin(2 * np.pi * 50.0 * np.arange(n) / SR)).astype(F32)


def random_cutoff(n, seed):
    """a fresh cutoff every frame, from [1, 0.45 sr]"""
    return np.random.default_rng(seed).uniform(1.0, 0.45 * SR, n).astype(F32)


# input / cutoff pairs: ( name, x( ch, n, seed ), cutoff( n, seed ) )
SIGNALS = (
    ("noise_1k", lambda ch, n, seed: noise(ch, n, seed), lambda n, seed: 1000.0),
    ("noise_sweep", lambda ch, n, seed: noise(ch, n, seed), lambda n, seed: sweep(n)),
    ("noise_wobble", lambda ch, n, seed: noise(ch, n, seed), lambda n, seed: wobble(n)),
    ("sine_random", lambda ch, n, seed: sine(ch, n), lambda n, seed: random_cutoff(n, seed)),
)


def _case(name, x, cutoff, kind, order, parity=True):
    assert x.shape[0] <= 3 and x.shape[1] <= N3
    return {"name": name, "x": x, "sr": SR, "cutoff": cutoff, "kind": kind, "order": order, "parity": parity}


def _make_cases():
    cases = []
    # every length; channel counts 1 / 2 / 3 in turn (with an odd n the later rows are not 16-byte aligned); odd and even orders
    by_length = ((BUTTERWORTH_LOW, 3), (BUTTERWORTH_HIGH, 4), (REPEAT_LOW, 16), (BUTTERWORTH_HIGH, 1), (BUTTERWORTH_LOW, 2), (REPEAT_HIGH, 16),
                 (BUTTERWORTH_LOW, 8), (BUTTERWORTH_HIGH, 3), (BUTTERWORTH_LOW, 4))
    for i, n in enumerate(LENGTHS):
        kind, order = by_length[i]
        sig = SIGNALS[1 + i % 3]
        cases.append(_case("n%d_%s%d_%s" % (n, KIND_NAMES[kind], order, sig[0]), sig[1](1 + i % 3, n, 100 + i), sig[2](n, 200 + i), kind, order))
    # every kind and order over three blocks, the four signals and the channel counts in turn
    i = 0
    for kind in (BUTTERWORTH_LOW, BUTTERWORTH_HIGH):
        for order in (0, 1, 2, 3, 4, 8):
            sig = SIGNALS[i % 4]
            cases.append(_case("%s%d_%s" % (KIND_NAMES[kind], order, sig[0]), sig[1](1 + i % 3, N3, 300 + i), sig[2](N3, 400 + i), kind, order))
            i += 1
    for kind in (REPEAT_LOW, REPEAT_HIGH):
        for order in (0, 1, 16):
            sig = SIGNALS[i % 4]
            ch, n = (1, BLOCK + 1) if order == 16 else (1 + i % 3, N3)
            cases.append(_case("%s%d_%s" % (KIND_NAMES[kind], order, sig[0]), sig[1](ch, n, 300 + i), sig[2](n, 400 + i), kind, order))
            i += 1
    # lengths that are multiples of 4, several blocks and channels: every row then starts on a 16-byte boundary and the device reads and
    # writes its runs 16 bytes at a time (the other lengths take scalar loads); one block exactly, and three with a tail that is whole quads
    quads = ((BLOCK, 2, BUTTERWORTH_LOW, 2, 2), (BLOCK, 3, BUTTERWORTH_HIGH, 3, 1), (BLOCK, 2, REPEAT_LOW, 16, 1),
             (N3 - 1, 3, BUTTERWORTH_LOW, 8, 1), (N3 - 1, 2, BUTTERWORTH_HIGH, 8, 3), (N3 - 1, 2, BUTTERWORTH_LOW, 3, 0),
             (N3 - 1, 3, BUTTERWORTH_HIGH, 2, 2), (N3 - 1, 2, REPEAT_HIGH, 3, 1))
    for j, (n, ch, kind, order, which) in enumerate(quads):
        assert n % 4 == 0
        sig = SIGNALS[which]
        cases.append(_case("n%d_%s%d_%s" % (n, KIND_NAMES[kind], order, sig[0]), sig[1](ch, n, 500 + j), sig[2](n, 600 + j), kind, order))
    # where the sequential fp32 loop stalls: a step under half an ulp of the state moves nothing
    cases.append(_case("dc_20hz_low2", np.full((2, N3), 0.5, F32), 20.0, BUTTERWORTH_LOW, 2))
    cases.append(_case("noise_1hz_low1", noise(1, N3, 7), 1.0, BUTTERWORTH_LOW, 1))
    # a NaN cutoff at one frame, and the same case without it
    curve = sweep(N3)
    cases.append(_case("clean_low3", noise(2, N3, 8), curve, BUTTERWORTH_LOW, 3))
    poisoned = curve.copy()
    poisoned[NAN_FRAME] = np.nan
    cases.append(_case("nan_low3", noise(2, N3, 8), poisoned, BUTTERWORTH_LOW, 3, parity=False))
    # sr / 2: the fp32 product lands past pi / 2, g = -2.3e7, the state map is s' = -s + ..., nothing decays: finiteness only
    cases.append(_case("nyquist_low3", noise(2, BLOCK + 1, 9), 24000.0, BUTTERWORTH_LOW, 3, parity=False))
    return cases


CASES = _make_cases()
IDS = [c["name"] for c in CASES]
PARITY_IDS = [c["name"] for c in CASES if c["parity"]]
assert len(set(IDS)) == len(IDS)


def case(name):
    return CASES[IDS.index(name)]


@functools.lru_cache(maxsize=None)
def expected(name, dtype=F32):
    """the sequential loop's output of a case in `dtype`, computed once and shared: treat as read-only"""
    c = case(name)
    out = filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"], dtype)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def stalls(name):
    """a case stalls when the fp32 loop itself is more than 1e-6 (rms or max) from the truth"""
    c = case(name)
    return max(errors(expected(name, F32), expected(name, F64), c["x"])) > 1e-6


# ---- rows longer than one pass of the carry kernel --------------------------------------------------------------------------------
# k_scan_carry (run_scan.h) scans 256 block totals in a pass and a block is 256 runs, so a pass is 65 536 runs: 65 536 frames at a run
# of 1, 1 048 576 at the default run.  These rows are not in CASES (which feeds the C ABI and host C++ modules and stops at N3); the
# device tests and the tests of the scan model build them here, once.
PASS_RUNS = 256 * 256
# at a run of 1: 256 blocks exactly, one pass; a second pass of one block of one frame; three passes, the third of 4 blocks, the last of 17 frames
LONG_RUN1 = (PASS_RUNS, PASS_RUNS + 1, 2 * PASS_RUNS + 3 * 256 + 17)
N_THREE_PASSES = LONG_RUN1[2]                          # 131 857
N_LONG = 257 * BLOCK + 16                              # 1 052 688 at the default run: 258 blocks, whole quads
assert N_LONG % 4 == 0 and N_THREE_PASSES == 131857 and N_LONG == 1052688


def windows(n, run):
    """[( label, lo, hi )]: the whole row, every pass's frames, and the first block (256 runs) of every pass after the first: where a
    state lost between passes shows before the filter has forgotten it"""
    per_pass = PASS_RUNS * run
    out = [("whole", 0, n)]
    for p, lo in enumerate(range(0, n, per_pass)):
        out.append(("pass %d" % p, lo, min(lo + per_pass, n)))
        if p:
            out.append(("pass %d head" % p, lo, min(lo + 256 * run, n)))
    return out


def errors_over(got, want, x, lo, hi):
    """errors() over frames [lo, hi) of every row, divided by the rms and the peak of the WHOLE input: a quiet stretch cannot inflate them"""
    d = np.asarray(got, F64)[:, lo:hi] - np.asarray(want, F64)[:, lo:hi]
    x = np.asarray(x, F64)
    return float(np.sqrt(np.mean(d * d))) / float(np.sqrt(np.mean(x * x))), float(np.max(np.abs(d))) / float(np.max(np.abs(x)))


def _long_table():
    table = {}
    for i, n in enumerate(LONG_RUN1):
        # order 3: a 1-pole section and a 2-pole section, so both maps cross the pass
        table["low3_n%d_run1" % n] = (BUTTERWORTH_LOW, 3, 3, n, 1, 1000 + i)
        table["high2_n%d_run1" % n] = (BUTTERWORTH_HIGH, 2, 3, n, 1, 1010 + i)
    table["rlow16_n%d_run1" % LONG_RUN1[1]] = (REPEAT_LOW, 16, 3, LONG_RUN1[1], 1, 1020)
    table["low3_n%d" % N_LONG] = (BUTTERWORTH_LOW, 3, 2, N_LONG, None, 1030)
    return table


LONG = _long_table()
LONG_IDS = list(LONG)


@functools.lru_cache(maxsize=None)
def long_case(name):
    """noise under the swept cutoff; run: the forced run the row is meant for (None: the library's choice).  Built once: read-only"""
    kind, order, ch, n, run, seed = LONG[name]
    x, cutoff = noise(ch, n, seed), sweep(n)
    x.setflags(write=False)
    cutoff.setflags(write=False)
    return {"name": name, "x": x, "sr": SR, "cutoff": cutoff, "kind": kind, "order": order, "run": run}


@functools.lru_cache(maxsize=None)
def long_expected(name, dtype=F32):
    """the sequential loop's output of a long case in `dtype`, computed once and shared: read-only"""
    c = long_case(name)
    out = filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"], dtype)
    out.setflags(write=False)
    return out


def figures(got, want, truth, x, run):
    """per window of windows(): ( label, vs the fp32 loop ( rms, max ), vs the truth ( rms, max ), the fp32 loop vs the truth ( rms, max ) )"""
    return [(label, errors_over(got, want, x, lo, hi), errors_over(got, truth, x, lo, hi), errors_over(want, truth, x, lo, hi))
            for label, lo, hi in windows(np.shape(x)[1], run)]


MEMORY_CUTOFF = 1.0                                    # Hz: the first-order low-pass forgets by exp( -2 pi / 48000 ) a frame, 1.9e-4 over a pass


def memory_inputs():
    """( x, other ) [3][131 857]: noise, and the same with frames [0, 256) replaced by a level of 24"""
    x = noise(3, N_THREE_PASSES, 1040)
    other = x.copy()
    other[:, :256] = F32(24)
    return x, other
