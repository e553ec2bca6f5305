"""Audio::compress (Audio/AudioVolume.cpp:190-278), Audio::modify_volume (:5-44) and Audio::set_volume (:46-67) restated in NumPy.
DESIGN.md 4.14.

    level()                  the per-frame part (:211-215, :264-269, :242): detector input, x_L, a_R, a_A, in fp32 or fp64
    peak_detector()          the sequential loop (:250-251) in fp32, one rounding per operation, or in fp64 (the "truth")
    peak_detector_scan()     the same recurrences as scans in fp64: a summary per run, composition, replay
    compress()               all of it: ( out, c )
    get_max_sample_magnitude / modify_volume / set_volume
    errors(), CASES
    LONG, long_case(), windows(), figures()
                             rows of more than 256 blocks, past one pass of the carry kernel, and the windows they are held over

log10, exp and pow of the fp32 loop are the fp64 functions rounded to fp32 once: what glibc's expf / powf return (they evaluate in
double), and what the device kernels do."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
RUN, WAVE, BLOCK = 16, 16 * 64, 16 * 256               # frames per lane, per wavefront, per block of compress.hip's scan


def _f(dtype, v):
    return np.asarray(v, F32).astype(dtype)              # parameters are fp32 values in either precision


def log10_of(x, dtype):
    return np.log10(x.astype(F64)).astype(dtype)


def exp_of(x, dtype):
    return np.exp(x.astype(F64)).astype(dtype)


def pow10_of(x, dtype):
    return np.power(10.0, x.astype(F64)).astype(dtype)


def detector_input(side, n):
    """:211-215: channel_max starts at 0 and takes a sample only if it is larger: the SIGNED maximum, no abs; NaN is never taken"""
    side = np.asarray(side, F32)
    x = np.zeros(n, F32)
    for c in range(side.shape[0]):
        s = side[c, :n]
        x = np.where(x < s, s, x)
    return x


def gain_computer(x_G, threshold, knee_width, ratio):
    """:227-239 in the precision of its arguments"""
    t = x_G.dtype.type
    with np.errstate(all="ignore"):
        overshoot = x_G - threshold
        slope = t(1) / ratio - t(1)
        before = overshoot <= -knee_width / t(2)
        after = overshoot >= knee_width / t(2)
        z = overshoot + knee_width / t(2)
        in_knee = x_G + slope * z * z / (t(2) * knee_width)
        return np.where(before, x_G, np.where(after, x_G + overshoot * slope, in_knee))


def level(x, sr, threshold, ratio, attack, release, knee_width, dtype=F32):
    """per frame: ( x_L, a_R, a_A ) from the detector input x [n]"""
    n = x.size
    p = [np.broadcast_to(_f(dtype, v), (n,)) for v in (threshold, ratio, attack, release, knee_width)]
    t = dtype
    x = np.asarray(x, F32).astype(dtype)
    sr = t(F32(sr))
    with np.errstate(all="ignore"):
        x_G = t(20) * log10_of(np.maximum(np.abs(x), t(F32(1e-6))), dtype)                 # :264
        y_G = gain_computer(x_G, p[0], p[4], p[1])
        x_L = x_G - y_G
        a_A = exp_of(t(-1) / (p[2] * sr), dtype)                                          # :242
        a_R = exp_of(t(-1) / (p[3] * sr), dtype)
    return x_L.astype(dtype), a_R, a_A


def peak_detector(x_L, a_R, a_A, dtype=F32):
    """:250-251, both states from 0 (:258-259): ( y_1, y_L ).  std::max( a, b ) is a < b ? b : a"""
    n = x_L.size
    y_1s, y_Ls = np.empty(n, dtype), np.empty(n, dtype)
    if dtype == F64:
        xs, rs, as_ = x_L.tolist(), a_R.tolist(), a_A.tolist()
        y_1 = y_L = 0.0
        for f in range(n):
            v = rs[f] * y_1 + (1.0 - rs[f]) * xs[f]
            y_1 = v if xs[f] < v else xs[f]
            y_L = as_[f] * y_L + (1.0 - as_[f]) * y_1
            y_1s[f], y_Ls[f] = y_1, y_L
        return y_1s, y_Ls
    one = F32(1)
    y_1 = y_L = F32(0)
    with np.errstate(all="ignore"):
        for f in range(n):
            x, r, a = x_L[f], a_R[f], a_A[f]                 # np.float32 scalars: every operation rounds to fp32
            v = r * y_1 + (one - r) * x
            y_1 = v if x < v else x
            y_L = a * y_L + (one - a) * y_1
            y_1s[f], y_Ls[f] = y_1, y_L
    return y_1s, y_Ls


# ---- the scan form ------------------------------------------------------------------------------------------------------------------
# stage 1: the maps y -> max( c, a y + b ), a >= 0, as ( a, b, c ); `later` after `earlier` is ( a2 a1, a2 b1 + b2, max( c2, a2 c1 + b2 ) );
# the identity is ( 1, 0, -inf ).  An empty floor stays empty whatever a2 is (0 x -inf has no value).
IDENTITY1 = (1.0, 0.0, -np.inf)
IDENTITY2 = (1.0, 0.0)


def then1(e, l):
    floor = -np.inf if e[2] == -np.inf else l[0] * e[2] + l[1]
    return (l[0] * e[0], l[0] * e[1] + l[1], max(l[2], floor))


def then2(e, l):
    return (l[0] * e[0], l[0] * e[1] + l[1])


def apply1(m, y):
    return max(m[2], m[0] * y + m[1])


def apply2(m, y):
    return m[0] * y + m[1]


def _scan(steps, run, then, identity, apply_map, replay_step):
    """steps: one map per frame.  A summary per run, an exclusive scan of the summaries, and a replay of every run from the state the
    scan carries in."""
    n = len(steps)
    starts = list(range(0, n, run))
    summaries = []
    for s in starts:
        m = identity
        for f in range(s, min(s + run, n)):
            m = then(m, steps[f])
        summaries.append(m)
    out = np.empty(n, F64)
    prefix = identity
    for k, s in enumerate(starts):
        y = apply_map(prefix, 0.0)
        for f in range(s, min(s + run, n)):
            y = replay_step(f, y)
            out[f] = y
        prefix = then(prefix, summaries[k])
    return out


def peak_detector_scan(x_L, a_R, a_A, run):
    """peak_detector( ..., F64 ) as two scans over runs of `run` frames, in fp64"""
    xs, rs, as_ = np.asarray(x_L, F64).tolist(), np.asarray(a_R, F64).tolist(), np.asarray(a_A, F64).tolist()
    n = len(xs)

    def step1(f, y):
        v = rs[f] * y + (1.0 - rs[f]) * xs[f]
        return v if xs[f] < v else xs[f]
    y_1 = _scan([(rs[f], (1.0 - rs[f]) * xs[f], xs[f]) for f in range(n)], run, then1, IDENTITY1, apply1, step1)
    y1s = y_1.tolist()
    y_L = _scan([(as_[f], (1.0 - as_[f]) * y1s[f]) for f in range(n)], run, then2, IDENTITY2, apply2,
                lambda f, y: as_[f] * y + (1.0 - as_[f]) * y1s[f])
    return y_1, y_L


def compress(audio, sr, sidechain=None, dtype=F32, threshold=-20.0, ratio=3.0, attack=0.005, release=0.1, knee_width=0.0):
    """Audio::compress: ( out [ch][n], c [n] ) in `dtype` (F32: the reference's loop; F64: the truth for the same fp32 inputs)"""
    audio = np.asarray(audio, F32)
    n = audio.shape[1]
    side = audio if sidechain is None else np.asarray(sidechain, F32)
    assert side.shape[1] >= n
    x_L, a_R, a_A = level(detector_input(side, n), sr, threshold, ratio, attack, release, knee_width, dtype)
    _, y_L = peak_detector(x_L, a_R, a_A, dtype)
    with np.errstate(all="ignore"):
        c = pow10_of(-y_L / dtype(20), dtype)                                            # :270-272
        return audio.astype(dtype) * c[None, :], c


def volume_end(n, sr):
    """AudioBuffer::get_max_sample_magnitude() with default arguments (AudioBuffer.cpp:416-430): frames [0, end),
    end = clamp( Frame( float( n ) / sr * sr ), 0, n - 1 ): the last frame is not looked at"""
    return int(min(max(int(F32(F32(n) / F32(sr)) * F32(sr)), 0), n - 1))


def get_max_sample_magnitude(x, sr):
    x = np.asarray(x, F32)
    end = volume_end(x.shape[1], sr)
    return F32(np.max(np.abs(x[:, :end]))) if end > 0 else F32(0)


def modify_volume(x, gain):
    """:32-44: one fp32 product per sample, gain a scalar or [n]"""
    return (np.asarray(x, F32) * np.broadcast_to(np.asarray(gain, F32), (np.shape(x)[1],))[None, :]).astype(F32)


def set_volume(x, sr, level_):
    """:56-67: m == 0 returns the input; else every sample times level[f] / m, one fp32 division and one fp32 product"""
    x = np.asarray(x, F32)
    m = get_max_sample_magnitude(x, sr)
    if m == 0:
        return x.copy()
    return modify_volume(x, np.broadcast_to(np.asarray(level_, F32), (x.shape[1],)) / m)


def errors(y, ref):
    """( relative rms error, max abs error / max |ref| )"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    d = y - ref
    scale = np.max(np.abs(ref)) if ref.size else 0.0
    if scale == 0.0:
        return (0.0, 0.0) if not np.any(d) else (np.inf, np.inf)
    return float(np.sqrt(np.sum(d * d) / np.sum(ref * ref))), float(np.max(np.abs(d)) / scale)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
SR = 48000.0
CONSTANTS = dict(threshold=-20.0, ratio=3.0, attack=0.005, release=0.1, knee_width=0.0)
LENGTHS = (1, 2, RUN - 1, RUN, RUN + 1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17)


def bursts(ch, n, seed):
    """noise bursts alternating -6 dB and -40 dB every 300 frames: both sides of the max and both time constants matter"""
    rng = np.random.default_rng(seed)
    amp = np.where((np.arange(n) // 300) % 2 == 0, 10.0 ** (-6 / 20), 10.0 ** (-40 / 20))
    return (rng.uniform(-1.0, 1.0, (ch, n)) * amp[None, :]).astype(F32)


def threshold_sweep(n):
    return np.linspace(-30.0, -10.0, n).astype(F32)


def attack_steps(n):
    """0.1 ms, 1 ms, 10 ms, 50 ms, a quarter of the signal each"""
    return np.asarray([0.0001, 0.001, 0.01, 0.05], F32)[np.minimum(np.arange(n) * 4 // max(n, 1), 3)]


def _case(name, x, side=None, **params):
    return {"name": name, "x": x, "side": side, "sr": SR, "params": dict(CONSTANTS, **params)}


def _make_cases():
    cases = []
    for i, n in enumerate(LENGTHS):                                  # every length, channel counts 1 / 2 / 3 in turn
        cases.append(_case("bursts_n%d" % n, bursts(1 + i % 3, n, 100 + i)))
    n = BLOCK + 1
    cases += [
        _case("knee6", bursts(2, n, 1), knee_width=6.0),
        _case("per_frame", bursts(2, n, 2), threshold=threshold_sweep(n), attack=attack_steps(n)),
        _case("per_frame_knee6_3blocks", bursts(1, 3 * BLOCK + 17, 3), threshold=threshold_sweep(3 * BLOCK + 17), attack=attack_steps(3 * BLOCK + 17), knee_width=6.0),
        _case("attack0", bursts(1, n, 4), attack=0.0),
        _case("release0", bursts(1, n, 5), release=0.0),
        _case("ratio1", bursts(2, n, 6), ratio=1.0),
        _case("ratio1e9", bursts(2, n, 7), ratio=1e9),
        _case("zeros", np.zeros((2, n), F32)),
        _case("dc", np.full((2, n), 0.5, F32)),
        _case("negative", -np.abs(bursts(3, n, 8)) - F32(1e-3)),
        _case("side_mono", bursts(3, n, 9), side=bursts(1, n, 10)),
        _case("side_longer", bursts(2, n, 11), side=bursts(2, n + 1000, 12), knee_width=6.0),
    ]
    return cases


CASES = _make_cases()
IDS = [c["name"] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


@functools.lru_cache(maxsize=None)
def expected(name, dtype=F32):
    """( out, c ) of a case, computed once and shared: treat as read-only"""
    c = case(name)
    out, gain = compress(c["x"], c["sr"], c["side"], dtype, **c["params"])
    out.setflags(write=False)
    gain.setflags(write=False)
    return out, gain


# ---- rows longer than one pass of the carry kernel --------------------------------------------------------------------------------
# k_scan_carry (run_scan.h) scans 256 block totals in a pass and a block is 256 runs, so a pass is 65 536 runs: 65 536 frames at a run
# of 1, 1 048 576 at the default run.  These rows are not in CASES (which feeds the C ABI and host C++ modules); the device tests and
# the tests of the scan form build them here, once.
PASS_RUNS = 256 * 256
# at a run of 1: 256 blocks exactly, one pass; a second pass of one block of one frame; three passes, the third of 4 blocks, the last of 17 frames
LONG_RUN1 = (PASS_RUNS, PASS_RUNS + 1, 2 * PASS_RUNS + 3 * 256 + 17)
N_THREE_PASSES = LONG_RUN1[2]                          # 131 857
N_LONG = 257 * BLOCK + 16                              # 1 052 688 at the default run: 258 blocks
assert N_THREE_PASSES == 131857 and N_LONG == 1052688


def windows(n, run):
    """[( label, lo, hi )]: the whole row, every pass's frames, and the first block (256 runs) of every pass after the first: where a
    state lost between passes shows before the release (0.1 s, 4800 frames) and the attack have let go of it"""
    per_pass = PASS_RUNS * run
    out = [("whole", 0, n)]
    for p, lo in enumerate(range(0, n, per_pass)):
        out.append(("pass %d" % p, lo, min(lo + per_pass, n)))
        if p:
            out.append(("pass %d head" % p, lo, min(lo + 256 * run, n)))
    return out


def errors_over(y, ref, lo, hi):
    """errors() over frames [lo, hi), divided by the rms and the peak of the WHOLE ref: a quiet stretch cannot inflate them"""
    y, ref = np.asarray(y, F64), np.asarray(ref, F64)
    d = y[..., lo:hi] - ref[..., lo:hi]
    return float(np.sqrt(np.mean(d * d) / np.mean(ref * ref))), float(np.max(np.abs(d)) / np.max(np.abs(ref)))


def figures(got, want, truth, run):
    """per window of windows(): ( label, vs the fp32 loop ( rms, max ), vs the truth ( rms, max ), the fp32 loop vs the truth ( rms, max ) )"""
    return [(label, errors_over(got, want, lo, hi), errors_over(got, truth, lo, hi), errors_over(want, truth, lo, hi))
            for label, lo, hi in windows(np.shape(want)[-1], run)]


LONG = dict([("bursts_n%d_run1" % n, (2, n, 1, 1200 + i)) for i, n in enumerate(LONG_RUN1)] + [("bursts_n%d" % N_LONG, (2, N_LONG, None, 1210))])
LONG_IDS = list(LONG)


@functools.lru_cache(maxsize=None)
def long_case(name):
    """bursts under the knee of 6 dB, the threshold sweep and the attack steps, the release at its default: 4800 frames of memory across
    a pass's boundary.  run: the forced run the row is meant for (None: the library's choice).  Built once: read-only"""
    ch, n, run, seed = LONG[name]
    c = _case(name, bursts(ch, n, seed), threshold=threshold_sweep(n), attack=attack_steps(n), knee_width=6.0)
    for v in (c["x"], c["params"]["threshold"], c["params"]["attack"]):
        v.setflags(write=False)
    return dict(c, run=run)


@functools.lru_cache(maxsize=None)
def long_expected(name, dtype=F32):
    """( out, c ) of a long case, computed once and shared: read-only"""
    c = long_case(name)
    out, gain = compress(c["x"], c["sr"], c["side"], dtype, **c["params"])
    out.setflags(write=False)
    gain.setflags(write=False)
    return out, gain
