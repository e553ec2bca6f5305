"""flan::Wavetable (Wavetable.cpp) restated in Python: the waveform starts (:19-65, :134-218), the Fourier resampling of a waveform
(:67-132), the table index (:463-488), Wavetable::synthesize's resampler loop (:266-334 over WDL_Resampler: tests/wdl_reference.py at
64 taps) and the four in-place edits (:364-451).  DESIGN.md 4.23.

resample_truth is fp64; resample_standin is the same around scipy.fft in single precision: not the reference's bits (FFTW's) but its
kind of error, as pitch_reference.d_standin is."""
import math
import os

import numpy as np

import wdl_reference as WDL

F32 = np.float32
TAPS, PRELUDE = 64, 31
SNAP_NONE, SNAP_ZERO, SNAP_LEVEL = 0, 1, 2
PITCH_NONE, PITCH_LOCAL, PITCH_GLOBAL = 0, 1, 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_made", "wdl_wavetable.npz")
GOLDEN_RUNS = os.path.join(os.path.dirname(GOLDEN), "wdl_wavetable_runs.npz")     # the cases that hold the run planner


# ---------------------------------------------------------------------------------------------------------------
# waveform starts

def trunc(v):
    """Frame( float )"""
    v = float(v)
    return 0 if v != v else int(v)


def snap(data, frame_to_snap, height, distance):
    """snap_frame_to_sample (:19-60), literally, in fp32"""
    data = np.asarray(data, F32)
    n = data.size
    height = F32(height)
    left_limit = max(frame_to_snap - distance, 0)
    right_limit = min(frame_to_snap + distance, n - 1)
    is_above = bool(data[frame_to_snap] > height)
    for offset in range(0, distance + 1):
        left = frame_to_snap - offset
        if left >= left_limit and bool(data[left] > height) != is_above:
            return left + 1
        right = frame_to_snap + offset
        if right < right_limit and bool(data[right] > height) != is_above:
            return right

    def norm(f):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = F32(F32(1.0) + F32(F32(1.0) * F32(abs(f - frame_to_snap))) / F32(distance))
            return F32(np.abs(F32(data[f] - height)) * r)

    best, best_d = frame_to_snap, norm(frame_to_snap)
    for f in range(left_limit, right_limit + 1):
        d = norm(f)
        if d < best_d:
            best, best_d = f, d
    return best


def starts(row, locals_, global_wavelength, snap_mode, pitch_mode, snap_ratio, fixed_frame):
    """the walk of :181-214 for one channel; pitch_mode is the mode in force for it"""
    row = np.asarray(row, F32)
    n = row.size
    snap_ratio = F32(snap_ratio)

    def handler(frame, source_frame, max_snap):
        if snap_mode == SNAP_ZERO:
            return snap(row, frame, 0.0, max_snap)
        if snap_mode == SNAP_LEVEL:
            return snap(row, frame, row[source_frame], max_snap)
        return frame

    out = [handler(0, 0, trunc(F32(snap_ratio * F32(global_wavelength))))]
    while True:
        if pitch_mode == PITCH_LOCAL:
            i = out[-1] // 128
            if i >= len(locals_):
                break
            local = trunc(locals_[i])
            expected = local if local > 0 else global_wavelength if global_wavelength > 0 else fixed_frame
        elif pitch_mode == PITCH_GLOBAL:
            expected = global_wavelength
        else:
            expected = fixed_frame
        if out[-1] + expected >= n:
            break
        assert expected >= 1 and len(out) <= 2 * n
        out.append(handler(out[-1] + expected, out[-1], trunc(F32(snap_ratio * F32(expected)))))
    return np.array(out, np.int32)


def table_index(starts_c, num_source_frames, r):
    """ratio_to_table_index (:463-488) in fp32 as written, for one value"""
    starts_c = [int(s) for s in starts_c]
    count = len(starts_c)
    source_frame = trunc(F32(F32(r) * F32(num_source_frames)))
    if source_frame <= 0:
        return F32(0)
    if source_frame > num_source_frames:
        return F32(count - 1)
    right = int(np.searchsorted(np.array(starts_c), source_frame, side="right"))       # upper_bound
    if right == 0:
        return F32(0)
    if right == count:
        return F32(count - 1)
    lo, hi = starts_c[right - 1], starts_c[right]
    index = F32(F32(right - 1) + F32(F32(source_frame - lo) / F32(hi - lo)))
    return F32(min(max(index, F32(0)), F32(count - 1)))


# ---------------------------------------------------------------------------------------------------------------
# table construction

def _search(y, W):
    """:105-120 -> ( zero_crossing_frame, the smallest |y| the search looked at, y[0] included )"""
    distance = int(F32(W) * F32(0.1))
    is_above = bool(y[0] > 0)
    margin = abs(float(y[0]))
    for offset in range(1, distance + 1):
        for t in (W - offset, offset):
            margin = min(margin, abs(float(y[t])))
            if bool(y[t] > 0) != is_above:
                return t, margin
    return 0, margin


def _resample(x, W, rfft, irfft, real, cplx):
    x = np.asarray(x, real)
    n = x.size
    X = rfft(x)
    Z = np.zeros(W // 2 + 1, cplx)
    k = min(X.size, Z.size)
    Z[:k] = X[:k]
    y = (irfft(Z, W) * real(W)).astype(real)                 # the unnormalised c2r (it ignores the imaginary parts of bins 0 and W/2)
    zc, margin = _search(y, W)
    return np.roll(y, -zc) / real(n), zc, margin, float(np.max(np.abs(y)))


def resample_truth(x, W):
    """one waveform in fp64 -> ( float64 [W] rotated and scaled, rotation, decision margin, max |y| ); margin and max are of the unscaled y"""
    return _resample(x, W, np.fft.rfft, np.fft.irfft, np.float64, np.complex128)


def resample_standin(x, W):
    """the same around scipy.fft in single precision (pocketfft keeps float32)"""
    import scipy.fft as sf
    return _resample(x, W, sf.rfft, sf.irfft, np.float32, np.complex64)


def build_table(audio, starts_list, W, one=resample_truth):
    """resample_waveforms over lists of starts: ( [ch][slots * W], rotations int [ch][slots], margins, maxima ); slots a channel does not fill
    (its last, and those of a shorter channel) and waveforms with n <= 0 stay 0"""
    ch = len(starts_list)
    slots = max(len(s) for s in starts_list)
    dtype = np.float64 if one is resample_truth else np.float32
    table = np.zeros((ch, slots * W), dtype)
    rot = np.zeros((ch, slots), np.int32)
    margins, maxima = np.full((ch, slots), np.inf), np.ones((ch, slots))
    for c, s in enumerate(starts_list):
        for w in range(len(s) - 1):
            n = int(s[w + 1]) - int(s[w])
            if n <= 0:
                continue
            table[c, w * W:(w + 1) * W], rot[c, w], margins[c, w], maxima[c, w] = one(audio[c, int(s[w]):int(s[w + 1])], W)
    return table, rot, margins, maxima


# ---------------------------------------------------------------------------------------------------------------
# synthesis

def synth_plan(out_frames, sr, W, g, freq):
    """The loop of :293-330 with the state of ResamplePrepare (:1218-1265) and ResampleOut (:1313-1343, :1558-1566) in fp64.  freq: the
    frequency per output frame (one entry: a constant).  ResampleOut is asked for all remaining frames, so a block ends where its input
    does.  One dict per block: offset, fracpos, ratio, filtpos, oversize, ideal, first_out, num_out, wanted, in_start."""
    freq = np.asarray(freq, F32).reshape(-1)
    rate_out = max(float(F32(sr)) / W, 1.0)
    blocks = []
    fracpos, S, offset, out, in_total, first = 0.0, 0, 0, 0, 0, True
    while out < out_frames:
        rate_in = max(float(freq[min(out, freq.size - 1)]), 1.0)
        ratio = rate_in / rate_out
        if S < PRELUDE:
            assert first, "the prelude is written once: S never drops below it again (ratio <= 34)"
            S = PRELUDE
        first = False
        wanted = max(int(ratio * g) + 4 + TAPS - S, 0)
        S += wanted
        filtpos, oversize, ideal = WDL.table_shape(rate_in, rate_out, ratio)
        limit = S - TAPS - 1
        srcpos, count = fracpos, 0
        while count < out_frames - out and int(srcpos) < limit:
            srcpos += ratio
            count += 1
        blocks.append(dict(offset=offset, fracpos=fracpos, ratio=ratio, filtpos=filtpos, oversize=oversize, ideal=int(ideal), first_out=out,
                           num_out=count, wanted=wanted, in_start=in_total))
        isrcpos = min(int(srcpos), S)
        fracpos = srcpos - isrcpos
        if ideal:
            fracpos = math.floor(oversize * fracpos + 0.5) / oversize
        S -= isrcpos
        offset += isrcpos
        in_total += wanted
        out += count
        assert count or wanted
    return blocks


def stream(tab, W, in_start, total_in, index_c, smooth, s):
    """stream samples s (an int64 array) of one channel: 31 zeros, then input sample t = s - 31 as the block that appended it blended it
    (:316-318), every operation rounded to fp32"""
    t = np.asarray(s, np.int64) - PRELUDE
    ok = (t >= 0) & (t < total_in)
    tc = np.where(ok, t, 0)
    q = np.searchsorted(in_start, tc, side="right") - 1
    idx = np.asarray(index_c, F32)[q]
    left, right = np.floor(idx).astype(np.int64), np.ceil(idx).astype(np.int64)
    rem = (idx - left.astype(F32)).astype(F32)
    phase = tc % W
    lv, rv = tab[phase + W * left], tab[phase + W * right]
    v = ((F32(1.0) - rem).astype(F32) * lv).astype(F32) + (rem * rv).astype(F32) if smooth else lv
    return np.where(ok, v.astype(F32), F32(0)).astype(F32)


def synth(table, W, sr, out_frames, g, freq, index, smooth=True, position="chain", blocks=None):
    """Wavetable::synthesize: table float32 [ch][slots * W], index float32 [ch][blocks] -> float32 [ch][out_frames].  position: "chain"
    forms srcpos by repeated += ratio like the reference, "fma" with one rounding like the device kernel."""
    table = np.asarray(table, F32)
    blocks = blocks or synth_plan(out_frames, sr, W, g, freq)
    in_start = np.array([b["in_start"] for b in blocks], np.int64)
    total_in = blocks[-1]["in_start"] + blocks[-1]["wanted"]
    ch = table.shape[0]
    out = np.zeros((ch, out_frames), F32)
    for b in blocks:
        m = b["num_out"]
        if not m:
            continue
        srcpos = WDL.positions(b["fracpos"], b["ratio"], m, position)
        length = int(srcpos[-1]) + TAPS + 1
        tab = WDL.table(b["filtpos"], b["oversize"], TAPS).reshape(b["oversize"] + 1, TAPS)
        for c in range(ch):
            buf = stream(table[c], W, in_start, total_in, index[c], smooth, b["offset"] + np.arange(length))
            out[c, b["first_out"]:b["first_out"] + m] = WDL.samples(srcpos, buf, tab, b["ideal"])
    return out


def block_index(starts_list, num_source_frames, ratio_frames, blocks):
    """float32 [ch][blocks]: table_index of the per-frame ratio at every block's first frame"""
    r = np.asarray(ratio_frames, F32).reshape(-1)
    return np.array([[table_index(s, num_source_frames, r[min(b["first_out"], r.size - 1)]) for b in blocks] for s in starts_list], F32)


def errors(y, ref):
    """( relative rms error, max abs error / max |ref| )"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    d = y - ref
    scale = np.max(np.abs(ref)) if ref.size else 0.0
    if scale == 0.0:
        return (0.0, 0.0) if not np.any(d) else (np.inf, np.inf)
    return float(np.sqrt(np.sum(d * d) / np.sum(ref * ref))), float(np.max(np.abs(d)) / scale)


def random_synth_case(seed):
    """the random shapes the planner tests and the device tests share: ( table, W, slots, frames, g, freq, ratio, smooth )"""
    rng = np.random.default_rng(seed)
    W = int(rng.choice([64, 128]))
    ch = int(rng.integers(1, 4))
    g = int(rng.choice([1, 7, 48, 480]))
    frames = int(rng.integers(1, 3001)) if g > 1 else int(rng.integers(1, 400))
    slots = int(rng.integers(2, 6))
    in_freq = 48000.0 / W
    kind = int(rng.integers(0, 3))
    t = np.arange(frames) / max(frames - 1, 1)
    if kind == 0:
        freq = np.full(frames, in_freq * rng.choice([0.25, 0.5, 1.0, 2.0, 3.0, 0.9, 1.7, 0.133]))
    elif kind == 1:
        lo, hi = sorted(rng.uniform(0.2, 6.0, 2))
        freq = in_freq * (lo + (hi - lo) * t)
    else:
        freq = in_freq * (1.0 + 0.6 * np.sin(2 * np.pi * rng.uniform(0.5, 4.0) * t))
    table = (0.5 * rng.standard_normal((ch, slots * W))).astype(F32)
    ratio = rng.uniform(0.0, 1.0, frames) if seed % 2 else t
    return table, W, slots, frames, g, freq.astype(F32), ratio.astype(F32), bool(seed % 3)


def load_cases(path=GOLDEN):
    """a reference-made fixture as a list of dicts"""
    z = np.load(path)
    cases = []
    for k, name in enumerate(z["names"]):
        sr, W, g, nout, smooth, blocks = z["meta_%d" % k]
        cases.append(dict(name=str(name), table=z["table_%d" % k], freq=z["freq_%d" % k], index=z["index_%d" % k], sr=float(sr), W=int(W),
                          g=int(g), out_frames=int(nout), smooth=bool(smooth), blocks=int(blocks), out=z["out_%d" % k],
                          wanted=z["wanted_%d" % k], delivered=z["delivered_%d" % k]))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# the in-place edits, per slot

def _slots(table, W, dtype):
    t = np.array(table, dtype)
    return t, t.reshape(-1, W)


def normalize(table, W):
    """:429-451 in fp32: the exact maximum, untouched below 0.001, else the division"""
    t, rows = _slots(table, W, F32)
    for r in rows:
        m = np.max(np.abs(r))
        if float(m) >= 0.001:
            r[:] = r / m
    return t


def remove_dc(table, W):
    """:414-427 in fp64"""
    t, rows = _slots(table, W, np.float64)
    rows -= rows.mean(axis=1, keepdims=True)
    return t


def _fade(frame, fade_frames):
    return math.sin(math.pi / 2.0 * (frame + 1) / fade_frames)


def add_fades(table, W, fade_frames):
    """:364-384 in fp64, every slot once"""
    t, rows = _slots(table, W, np.float64)
    for frame in range(min(fade_frames - 1, W)):
        rows[:, frame] *= _fade(frame, fade_frames)
        rows[:, W - 1 - frame] *= _fade(frame, fade_frames)
    return t


def remove_jumps(table, W, fade_frames):
    """:386-412 in fp64, every slot once"""
    t, rows = _slots(table, W, np.float64)
    mid = (rows[:, 0] + rows[:, W - 1]) / 2.0
    for frame in range(min(fade_frames - 1, W)):
        for f in (frame, W - 1 - frame):
            rows[:, f] = (rows[:, f] - mid) * _fade(frame, fade_frames) + mid
    return t


# ---------------------------------------------------------------------------------------------------------------
# the resample cases the cpu and gpu tests share

RESAMPLE_FRAMES = 6000
RESAMPLE_W = (64, 256, 2048)


def resample_signals():
    """( a three-harmonic 217.3 Hz tone, Gaussian noise ), float32 [2][6000] at 48 kHz"""
    t = np.arange(RESAMPLE_FRAMES) / 48000.0
    tone = 0.5 * np.sin(2 * np.pi * 217.3 * t + 0.3) + 0.25 * np.sin(2 * np.pi * 2 * 217.3 * t + 1.1) + 0.125 * np.sin(2 * np.pi * 3 * 217.3 * t + 2.0)
    noise = 0.3 * np.random.default_rng(77).standard_normal(RESAMPLE_FRAMES)
    return np.array([tone, noise], F32)


def resample_lengths(W):
    return [1, 2, 3, 7, 100, 221, W - 1, W, W + 1, 2 * W]


def resample_case(W):
    """( audio float32 [ch][6000], one start list per channel ): the lengths of resample_lengths( W ), and one n = 0, packed into as few
    start lists as fit 6000 frames (two at least, of different lengths), each list over both signals"""
    lists, cur = [], [3]
    for n in sorted(resample_lengths(W), reverse=True):
        if cur[-1] + n > RESAMPLE_FRAMES - 1:
            lists.append(cur)
            cur = [3]
        cur.append(cur[-1] + n)
    lists.append(cur)
    if len(lists) == 1:
        k = len(cur) // 2 + 1
        lists = [cur[:k], [s - cur[k - 1] + 11 for s in cur[k - 1:]]]
    lists[-1] = lists[-1] + [lists[-1][-1], lists[-1][-1] + 5]          # a repeated start: n = 0, then n = 5
    signals = resample_signals()
    audio = np.array([signals[s] for _ in lists for s in range(2)], F32)
    starts_list = [list(l) for l in lists for _ in range(2)]
    return audio, starts_list
