"""The YIN pitch tracker of Audio::get_local_wavelengths (Audio/AudioInformation.cpp:18-75, 138-265; DSPUtility.cpp:37-185) restated in
NumPy, for tests/test_pitch_*.py and tests/test_gpu_pitch.py.  The reference itself cannot be built for this family (it needs FFTW), so
nothing here was made by it.

  d_truth      the difference function as its definition, in fp64: the truth
  d_standin    compute_d as the reference runs it -- fp32 power terms, two fp32 FFTs, p0 + p_tau - 2 r[tau] -- around SciPy's single
               precision FFT instead of FFTW's: not the reference's bits, but its kind and size of error; used only to measure that
  dprime       compute_d_prime: d rounded to fp32 (the reference's d is fp32), a running double sum, one rounding to fp32
  valleys      find_valleys( d' ) with its defaults, vectorised over runs of equal values; valleys_literal is the reference's walk from
               every point, kept to check the former against
  pick         the selection of get_local_wavelength; pick_branch also says which way it went
  continuity   the octave-continuity pass of get_local_wavelengths, as written
  average      get_average_wavelength( locals, ... ) with mean_and_sd in fp32, in order
  count        the number of analysis windows
A d' row with a NaN or an infinity answers 0, as the device does (include/flanhip.h says why)."""
import functools

import numpy as np
import scipy.fft

F32, F64 = np.float32, np.float64


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool(np.all(a.view(np.uint32) == b.view(np.uint32)))


# ---- windows ----------------------------------------------------------------------------------------------------------------------

def window_starts(num_frames, start=0, end=-1, window=2048, hop=128):
    """:180-183: start, start + hop, ... while frame + window < end"""
    if end == -1:
        end = num_frames
    out, frame = [], start
    while frame + window < end:
        out.append(frame)
        frame += hop
    return out


def count(num_frames, start=0, end=-1, window=2048, hop=128):
    return len(window_starts(num_frames, start, end, window, hop))


# ---- d ----------------------------------------------------------------------------------------------------------------------------

def d_truth(xw):
    """xw: the n samples of a window -> d[tau] = sum_{i<h} ( x[i] - x[i+tau] )^2, tau < h = n // 2, in fp64"""
    x = np.asarray(xw, F64)
    h = x.size // 2
    if h == 0:
        return np.zeros(0, F64)
    lagged = np.lib.stride_tricks.sliding_window_view(x, h)[:h]              # [tau][i] = x[tau + i]
    diff = lagged - x[:h]
    return np.einsum("ti,ti->t", diff, diff)


def d_standin(xw):
    """compute_d (:18-57) in fp32 around a single precision FFT"""
    x = np.ascontiguousarray(xw, F32)
    n = x.size
    h = n // 2
    if h == 0:
        return np.zeros(0, F32)
    sq = x * x
    p0 = np.cumsum(sq[:h], dtype=F32)[-1]                                    # :25-27, in order
    steps = np.empty(2 * h - 1, F32)                                         # :28-29: ( p - in[tau-1]^2 ) + in[tau-1+h]^2, in order
    steps[0] = p0
    steps[1::2] = -sq[:h - 1]
    steps[2::2] = sq[h:2 * h - 1]
    power = np.cumsum(steps, dtype=F32)[0::2]
    half = np.zeros(n, F32)
    half[:h] = x[:h]
    spectrum = scipy.fft.rfft(x) * np.conj(scipy.fft.rfft(half))             # complex64
    assert spectrum.dtype == np.complex64
    r = scipy.fft.irfft(spectrum, n)[:h].astype(F32)                          # normalised: the reference's buffer / n (:54)
    return ((p0 + power) - F32(2) * r).astype(F32)


def dprime(d):
    """compute_d_prime (:59-75) of d (rounded to fp32 first)"""
    d32 = np.asarray(d).astype(F32)
    h = d32.size
    out = np.ones(h, F32)
    if h < 2:
        return out
    d64 = d32[1:].astype(F64)
    total = np.cumsum(d64)                                                    # sequential, as the reference's loop
    live = total != 0
    tau = np.arange(1, h, dtype=F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out[1:] = np.where(live, (d64 * (tau / total)).astype(F32), F32(1))
    return out


# ---- valleys ----------------------------------------------------------------------------------------------------------------------

def _parabola(d0, d1, d2, x1):
    """DSPUtility.cpp:37-43 on -d' (arrays of fp32), y negated back (:139-140)"""
    y0, y1, y2 = -d0, -d1, -d2
    delta = F32(0.5) * (y0 - y2) / (y0 - F32(2) * y1 + y2)
    X = x1.astype(F32) + delta
    Y = -(y1 - F32(0.25) * (y0 - y2) * delta)
    return X.astype(F32), Y.astype(F32)


def valleys(dp):
    """( x, y ) of find_valleys( d' ) with its defaults, ordered by x; dp finite"""
    dp = np.ascontiguousarray(dp, F32)
    h = dp.size
    if h < 3:
        return np.zeros(0, F32), np.zeros(0, F32)
    change = np.flatnonzero(dp[1:] != dp[:-1]) + 1
    s = np.concatenate([[0], change])                                         # runs of equal values [s, e]
    e = np.concatenate([change - 1, [h - 1]])
    keep = (s >= 1) & (e <= h - 2)
    s, e = s[keep], e[keep]
    keep = (dp[s - 1] > dp[s]) & (dp[e + 1] > dp[e])
    s, e = s[keep], e[keep]
    single = s == e
    X, Y = np.empty(s.size, F32), np.empty(s.size, F32)
    with np.errstate(all="ignore"):
        X[single], Y[single] = _parabola(dp[s[single] - 1], dp[s[single]], dp[s[single] + 1], s[single])
    left, right = s[~single] - 1, e[~single] + 1                              # :93-103: a plateau
    X[~single] = ((right + left) * 0.5).astype(F32)
    Y[~single] = dp[s[~single]]
    return X, Y


def valleys_literal(dp):
    """the reference's own walk (DSPUtility.cpp:55-147), point by point; a list of ( x, y ) ordered by x"""
    dp = np.ascontiguousarray(dp, F32)
    size = dp.size
    data = -dp
    peaks = []
    if size < 2:
        return peaks
    for frame in range(1, size - 1):
        val = data[frame]

        def finder(go_right):
            new = frame
            while True:
                new += 1 if go_right else -1
                if new < 0 or size <= new:
                    return -1
                if data[new] > val:
                    return -1
                if data[new] < val:
                    return new

        left = finder(False)
        if left == -1:
            continue
        right = finder(True)
        if right == -1:
            continue
        if right - left > 2:
            mean = (right + left) * 0.5
            if frame != np.floor(mean):
                continue
            peaks.append((F32(mean), F32(-val)))
        else:
            y0, y1, y2 = data[frame - 1], data[frame], data[frame + 1]
            with np.errstate(all="ignore"):
                delta = F32(0.5) * (y0 - y2) / (y0 - F32(2) * y1 + y2)
                X = F32(frame) + delta
                Y = y1 - F32(0.25) * (y0 - y2) * delta
            peaks.append((F32(X), F32(-Y)))
    peaks.sort(key=lambda p: p[0])
    return peaks[:size // 2]


# ---- the selection ----------------------------------------------------------------------------------------------------------------

def select(X, Y, absolute_cutoff=0.2, minimum_wavelength=10):
    """AudioInformation.cpp:149-165 over the valleys ( X, Y ) -> ( wavelength, branch ): branch is "none" (no valley beyond the minimum
    wavelength), "nothing" (no valley below lowest.y * 2: lowest.y <= 0), "lowest" (the lowest valley itself) or "earlier" (an earlier one
    within the factor 2), with "+cutoff" behind it where the cutoff turned the answer into 0"""
    valid = np.flatnonzero(F32(minimum_wavelength) < X)
    if valid.size == 0:
        return F32(0), "none"
    k = int(valid[0])                                                         # X ascends: upper_bound
    lowest = k + int(np.argmin(Y[k:]))                                        # the first minimum
    with np.errstate(all="ignore"):
        limit = Y[lowest] * F32(2)
    under = np.flatnonzero(Y[k:] < limit)
    if under.size == 0:
        best_x, best_y, branch = F32(0), F32(0), "nothing"
    else:
        best = k + int(under[0])
        best_x, best_y, branch = X[best], Y[best], "lowest" if best == lowest else "earlier"
    if best_y < F32(absolute_cutoff):
        return F32(best_x), branch
    return F32(0), branch + "+cutoff"


def pick_branch(dp, absolute_cutoff=0.2, minimum_wavelength=10):
    dp = np.ascontiguousarray(dp, F32)
    if not np.all(np.isfinite(dp)):
        return F32(0), "nonfinite"
    return select(*valleys(dp), absolute_cutoff, minimum_wavelength)


def pick(dp, absolute_cutoff=0.2, minimum_wavelength=10):
    """get_local_wavelength's answer for the d' row dp"""
    return pick_branch(dp, absolute_cutoff, minimum_wavelength)[0]


def pick_literal(dp, absolute_cutoff=0.2, minimum_wavelength=10):
    """the same over valleys_literal, with the reference's loops"""
    minima = valleys_literal(dp)
    k = next((i for i, m in enumerate(minima) if F32(minimum_wavelength) < m[0]), None)
    if k is None:
        return F32(0)
    lowest = minima[k]
    for m in minima[k:]:
        if m[1] < lowest[1]:
            lowest = m
    best = (F32(0), F32(0))
    for i in range(len(minima) - 1, k - 1, -1):
        if minima[i][1] < lowest[1] * F32(2):
            best = minima[i]
    return F32(best[0]) if best[1] < F32(absolute_cutoff) else F32(0)


# ---- the host passes --------------------------------------------------------------------------------------------------------------

def continuity(w, sample_rate, hop_size):
    """AudioInformation.cpp:190-226 on a copy of w"""
    out = np.array(w, F32).reshape(-1)
    size = out.size
    if size == 0:
        return out
    minimum_num_hops = int((F32(0.1) * F32(sample_rate)) / F32(hop_size))
    sus_hops = []
    with np.errstate(all="ignore"):
        for i in range(size - 1):
            if out[i] == 0:
                continue
            r = float(out[i + 1] / out[i])                                    # an fp32 quotient against double literals
            if 1.95 < r and r < 2.05:
                sus_hops.append(i + 1)
        for hop in sus_hops:
            sus_length = 0
            while True:                                                       # do { ... } while( ++sus_length <= minimum_num_hops )
                global_hop = hop + sus_length
                if global_hop >= size:
                    break
                if out[global_hop] != 0:                                      # ( == 0: `continue`, to the condition )
                    r = out[global_hop] / out[hop]
                    if r < F32(0.95) or r > F32(1.05):
                        break
                sus_length += 1
                if not sus_length <= minimum_num_hops:
                    break
            if sus_length > minimum_num_hops:
                break
            out[hop:hop + sus_length] = out[hop:hop + sus_length] / F32(2)
    return out


def average(locals_, min_active_ratio=0.0, max_length_sigma=-1.0):
    """:245-265 and mean_and_sd (DSPUtility.cpp:159-185)"""
    w = np.asarray(locals_, F32).reshape(-1)
    num_valids = int(w.size - np.count_nonzero(w == F32(-1)))
    if F32(num_valids) <= F32(min_active_ratio) * F32(w.size):
        return F32(-1)
    valid = w[w != 0]
    mean, sd = F32(0), F32(0)
    if valid.size:
        with np.errstate(all="ignore"):
            mean = np.cumsum(valid, dtype=F32)[-1] / F32(valid.size)
            diff = valid - mean
            sd = np.sqrt(np.cumsum(diff * diff, dtype=F32)[-1] / F32(valid.size))
    if F32(max_length_sigma) != F32(-1) and sd > F32(max_length_sigma):
        return F32(-1)
    return F32(mean)


# ---- crafted rows and vectors -----------------------------------------------------------------------------------------------------
# d' rows, one per branch of the pick; ( row, absolute_cutoff, minimum_wavelength, the answer by hand or None )
def _row(*values):
    return np.array(values, F32)


PICK_ROWS = {
    # no interior point is a valley: monotone
    "no_valley": (_row(1, .9, .8, .7, .6, .5, .4, .3), 0.2, 1, 0.0),
    # one valley at exactly x = 4 (symmetric neighbours: delta = 0): minimum_wavelength 4 is not below it, 3 is
    "x_equals_minimum": (_row(1, 1, 1, .5, .1, .5, 1, 1), 0.2, 4, 0.0),
    "x_above_minimum": (_row(1, 1, 1, .5, .1, .5, 1, 1), 0.2, 3, 4.0),
    # a plateau of two points (3, 4): left 2, right 5, mean 3.5, the point 3 counts; of three points (3, 4, 5): mean 4
    "plateau_even": (_row(1, 1, .5, .1, .1, .5, 1, 1), 0.2, 1, 3.5),
    "plateau_odd": (_row(1, 1, .5, .1, .1, .1, .5, 1, 1), 0.2, 1, 4.0),
    # a flat stretch running into the right edge, and one into the left edge: neither is a valley; the true valley at 3 is
    "flat_into_right_edge": (_row(1, 1, .5, .15, .5, .05, .05, .05), 0.2, 1, 3.0),
    "flat_into_left_edge": (_row(.05, .05, .05, .5, 1, .5, .15, .5, 1), 0.2, 1, 6.0),
    # the lowest valley has y <= 0: y < lowest.y * 2 holds for nothing, the answer is 0
    "lowest_nonpositive": (_row(1, 1, .5, 0, .5, 1, .5, .1, .5, 1), 0.2, 1, 0.0),
    "lowest_negative": (_row(1, 1, .5, -.25, .5, 1, .5, .1, .5, 1), 0.2, 1, 0.0),
    # the lowest valley is at 7 (y .1); the one at 3 (y .15 < .2) is earlier and within the factor 2: chosen
    "earlier_within_factor": (_row(1, 1, .5, .15, .5, 1, .5, .1, .5, 1), 0.2, 1, 3.0),
    # the same with the earlier one too high (.25 >= .2): the lowest itself
    "earlier_too_high": (_row(1, 1, .5, .25, .5, 1, .5, .1, .5, 1), 0.2, 1, 7.0),
    # the only valley is .3: the cutoff .2 refuses it, the cutoff .35 does not
    "cutoff_fails": (_row(1, 1, .6, .3, .6, 1, 1, 1), 0.2, 1, 0.0),
    "cutoff_passes": (_row(1, 1, .6, .3, .6, 1, 1, 1), 0.35, 1, 3.0),
    # an asymmetric valley: the interpolated position and depth
    "interpolated": (_row(1, 1, .7, .2, .4, 1, 1, 1), 0.5, 1, None),
    # silence: d' == 1 everywhere, every walk ends at an edge
    "all_ones": (np.ones(64, F32), 0.2, 1, 0.0),
    # the smallest row with an interior point
    "h3_valley": (_row(1, .1, 1), 0.2, 0, 1.0),
    "h3_none": (_row(1, .1, .1), 0.2, 0, 0.0),
    # a NaN and an infinity: 0
    "nan": (_row(1, 1, .5, np.nan, .5, .1, .5, 1), 0.2, 1, 0.0),
    "inf": (_row(1, 1, .5, .1, .5, np.inf, .5, 1), 0.2, 1, 0.0),
}

# wavelength vectors for the continuity pass at 48 kHz, hop 128: minimum_num_hops = int( 4800 / 128 ) = 37
CONTINUITY_SR, CONTINUITY_HOP, CONTINUITY_MIN_HOPS = 48000.0, 128, 37


def _vector(*parts):
    return np.concatenate([np.full(n, v, F32) for v, n in parts])


CONTINUITY_VECTORS = {
    # five hops an octave down inside a long note: halved
    "short_doubling": _vector((100, 20), (200, 5), (100, 20)),
    # 38 hops: one more than the note length, a new note; it stays, and the pass ENDS: the short doubling behind it stays too
    "long_doubling_stops_the_pass": _vector((100, 10), (200, 38), (100, 10), (200, 3), (100, 10)),
    # exactly minimum_num_hops: still halved
    "doubling_of_the_note_length": _vector((100, 10), (200, 37), (100, 10)),
    # zeros inside the doubled run are counted and skipped; zeros between the notes hide a doubling from the search
    "zeros_inside_a_run": _vector((100, 10), (200, 2), (0, 3), (200, 2), (100, 10)),
    "zeros_before_a_doubling": _vector((100, 10), (0, 2), (200, 4), (100, 10)),
    # a doubling at the very last element
    "doubling_at_the_end": _vector((100, 10), (200, 1)),
    # two short doublings, and a second one whose ratio is taken against an already halved value
    "two_doublings": _vector((100, 10), (200, 4), (100, 10), (201, 3), (100, 10)),
    "doubling_of_a_doubling": _vector((100, 10), (200, 4), (400, 4), (100, 10)),
    "single": _vector((100, 1)),
    "all_zero": _vector((0, 12)),
}


def random_wavelengths(seed):
    """a seeded vector of the kind the pass meets: a note with jitter, octave jumps of random length (zeros and drop-outs inside some of
    them), other notes, zeros, -1"""
    rng = np.random.default_rng(seed)
    base = float(rng.uniform(40, 400))

    def run(value, length):
        v = np.full(length, value, F64)
        return v * rng.uniform(.985, 1.015, length) if value > 0 else v

    parts = [run(base, int(rng.integers(1, 30)))]
    for _ in range(int(rng.integers(1, 7))):
        kind = int(rng.integers(0, 6))
        if kind <= 2:                                                      # an octave down and back, short or long
            doubled = run(2 * base, int(rng.integers(1, 70 if kind == 2 else 12)))
            if kind == 1 and doubled.size > 2:
                doubled[int(rng.integers(1, doubled.size))] = 0.0
            parts += [doubled, run(base, int(rng.integers(1, 30)))]
        elif kind == 3:
            parts.append(run(0.0, int(rng.integers(1, 8))))
        elif kind == 4:
            parts.append(run(base * float(rng.uniform(.5, 2.2)), int(rng.integers(1, 30))))
        else:
            parts.append(run(-1.0, int(rng.integers(1, 4))))
    return np.concatenate(parts).astype(F32)


# ---- the GPU suite's signals ------------------------------------------------------------------------------------------------------
SR = 48000.0
SIGNALS = ("tone220", "tone97", "glide", "weak_fundamental", "high_pair", "noise")


@functools.lru_cache(maxsize=None)
def signal(name, frames):
    """48 kHz fp32; rng( 11 ) noise of sigma .02 under every tone (noise alone: sigma .3); "zeros" and "dc" are clean"""
    t = np.arange(frames, dtype=F64) / SR
    floor = np.random.default_rng(11).normal(0.0, 1.0, frames)
    two_pi = 2 * np.pi
    if name == "zeros":
        x = np.zeros(frames)
    elif name == "dc":
        x = np.full(frames, 0.25)
    elif name == "noise":
        x = 0.3 * floor
    else:
        if name == "tone220":
            x = 0.35 * sum(np.sin(two_pi * 220.0 * k * t + k) / k for k in range(1, 6)) / 1.5
        elif name == "tone97":
            x = 0.35 * sum(np.sin(two_pi * 97.3 * k * t + 0.5 * k) / k for k in range(1, 6)) / 1.5
        elif name == "glide":
            phase = two_pi * (220.0 * t + 0.5 * (220.0 / (frames / SR)) * t * t)        # 220 -> 440 Hz over the signal
            x = 0.3 * np.sin(phase) + 0.1 * np.sin(2 * phase)
        elif name == "weak_fundamental":
            x = 0.06 * np.sin(two_pi * 150.0 * t) + 0.3 * np.sin(two_pi * 300.0 * t + 1.0)
        elif name == "high_pair":
            x = 0.25 * np.sin(two_pi * 1600.0 * t) + 0.15 * np.sin(two_pi * 3200.0 * t + 0.3)
        else:
            raise KeyError(name)
        x = x + 0.02 * floor
    x = x.astype(F32)
    x.setflags(write=False)
    return x


# ( window, hop, frames, start, end )
SHAPES = {
    "default": (2048, 128, 16000, 0, -1),
    "w256": (256, 32, 3000, 0, -1),
    "w64": (64, 16, 1200, 0, -1),
    "odd101": (101, 25, 1500, 0, -1),
    "h3": (6, 1, 40, 0, -1),
    "inner_range": (256, 32, 3000, 77, 2501),
}
LARGER = ("default", "w256", "w64", "odd101")


@functools.lru_cache(maxsize=None)
def truth(name, shape):
    """Everything the tests need of one ( signal, shape ), computed once and never changed: the windows' starts, d' of the truth and of the
    stand-in (fp32 [W][h]), the raw picks of both with the truth's branches, and the truth's wavelengths after the continuity pass"""
    window, hop, frames, start, end = SHAPES[shape]
    x = signal(name, frames)
    starts = window_starts(frames, start, end, window, hop)
    dp_t = np.array([dprime(d_truth(x[s:s + window])) for s in starts], F32).reshape(len(starts), window // 2)
    dp_s = np.array([dprime(d_standin(x[s:s + window])) for s in starts], F32).reshape(len(starts), window // 2)
    picked = [pick_branch(row) for row in dp_t]
    out = {
        "x": x, "starts": starts, "dprime": dp_t, "dprime_standin": dp_s,
        "raw": np.array([p[0] for p in picked], F32), "branches": [p[1] for p in picked],
        "raw_standin": np.array([pick(row) for row in dp_s], F32),
    }
    out["wavelengths"] = continuity(out["raw"], SR, hop)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def disagreement(a, b):
    """per window: one is zero and the other is not, or the relative difference exceeds 1e-3 -> ( excluded mask, relative deviation where
    both are non-zero )"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    both = (a != 0) & (b != 0)
    rel = np.zeros(a.shape, F64)
    rel[both] = np.abs(a[both] - b[both]) / np.abs(b[both])
    return ((a == 0) != (b == 0)) | (rel > 1e-3), rel
