"""Audio::mix and the granular family over it, restated in NumPy from the reference's sources (Audio/AudioCombination.cpp:102-170,
Audio/AudioSynthesis.cpp:310-374, 572-638, Audio/AudioTemporal.cpp:190-234, Audio/AudioVolume.cpp:102-135, WindowFunctions.cpp:10-13):

  events( ... )        integrate_event_rate without scatter: the fp32 accumulator from 1.0f
  cut( ... ), cut_frames( ... )    Audio::cut's validation: truncation, end <= start before the clamp, the clamp, the fade rescale
  plan( ... )          the output's length max( o + n ) and, per tile, the first and last event index that touch it
  terms32( ... )       one event's terms in fp32, operation by operation, with the double cos of hann
  mix32( ... )         the ordered fp32 sum from +0.0f, one addition per term, in ascending event index: what the reference's loop computes
  mix64( ... )         the same sum in fp64 over terms computed in fp64 from the same fp32 inputs: the truth

An event table is a NumPy record array of EVENT, field for field the C ABI's flanhip_grain_event; `src` is an offset in floats into one flat
array of sources."""
import numpy as np

F32 = np.float32
EVENT = np.dtype([("src", np.uint64), ("ch_stride", np.int64), ("src_frames", np.int64), ("o", np.int64), ("gain_offset", np.int64),
                  ("s", np.int32), ("n", np.int32), ("channels", np.int32), ("sf", np.int32), ("ef", np.int32), ("flags", np.int32),
                  ("gain", np.float32), ("reserved", np.int32)], align=True)
HANN = 1
TWO_PI_F32 = F32(2.0) * F32(np.arccos(F32(-1.0)))             # 2.0f * pi, pi = std::acos( -1.0f )


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def make_events(count):
    e = np.zeros(count, EVENT)
    e["gain_offset"] = -1
    e["gain"] = 1.0
    return e


# ---- integrate_event_rate (AudioSynthesis.cpp:310-374), scatter 0 -----------------------------------------------------------------------
def events(length_frames, sample_rate, rate):
    """rate: a number or length_frames floats.  The event frames, int64"""
    sr = F32(sample_rate)
    r = np.maximum(F32(0), np.broadcast_to(np.asarray(rate, F32), (length_frames,)))       # :320
    inc = r / sr
    out = []
    acc = F32(1.0)                                              # :328
    for frame in range(length_frames):
        acc = F32(acc + inc[frame])
        if acc >= F32(1.0):
            out.append(frame)
            acc = F32(acc - np.floor(acc))
    return np.array(out, np.int64)


def event_time(frame, sample_rate):
    """:371: frame / sample_rate in fp32"""
    return F32(F32(frame) / F32(sample_rate))


def time_to_frame(t, sample_rate):
    """time_to_frame( t ) truncated to Frame, or None where no Frame holds it"""
    with np.errstate(all="ignore"):
        f = F32(F32(t) * F32(sample_rate))
    if not (f > F32(-2147483648.0) and f < F32(2147483648.0)):
        return None
    return int(f)


# ---- Audio::cut / cut_frames -----------------------------------------------------------------------------------------------------------
def cut_frames(num_frames, start, end, start_fade, end_fade):
    """( s, n, sf, ef ); n == 0: the null Audio"""
    if end <= start:                                            # AudioTemporal.cpp:217
        return 0, 0, 0, 0
    start = min(max(start, 0), num_frames - 1)                 # :218-219
    end = min(max(end, 0), num_frames - 1)
    n = end - start
    if n <= 0:
        return 0, 0, 0, 0
    sf, ef = max(0, start_fade), max(0, end_fade)              # AudioVolume.cpp:111-112
    if sf + ef > n:
        scale = F32(F32(n) / F32(sf + ef))                     # :115-117
        sf = int(np.floor(F32(F32(sf) * scale)))
        ef = int(np.floor(F32(F32(ef) * scale)))
    return start, n, sf, ef


def cut(num_frames, sample_rate, start_time, end_time, start_fade, end_fade):
    frames = [time_to_frame(t, sample_rate) for t in (start_time, end_time, start_fade, end_fade)]
    if any(f is None for f in frames):
        return 0, 0, 0, 0
    return cut_frames(num_frames, *frames)


def cut_table(num_frames, sample_rate, start_time, end_time, start_fade, end_fade):
    e = make_events(len(start_time))
    for i in range(len(start_time)):
        e["s"][i], e["n"][i], e["sf"][i], e["ef"][i] = cut(num_frames, sample_rate, start_time[i], end_time[i], start_fade[i], end_fade[i])
    return e


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------
def out_frames(ev):
    return int(max([0] + [int(e["o"]) + int(e["n"]) for e in ev]))       # AudioCombination.cpp:146-150


def plan(ev, tile, frames=None):
    frames = out_frames(ev) if frames is None else frames
    tiles = -(-frames // tile)
    first, last = np.zeros(tiles, np.int32), np.full(tiles, -1, np.int32)
    for t in range(tiles):
        lo, hi = t * tile, min((t + 1) * tile, frames)
        hit = [i for i, e in enumerate(ev) if e["n"] > 0 and e["channels"] > 0 and e["o"] < hi and e["o"] + e["n"] > lo]
        if hit:
            first[t], last[t] = hit[0], hit[-1]
    return frames, first, last


# ---- the terms and the sums ----------------------------------------------------------------------------------------------------------------
def _source(e, sources, channel):
    at = int(e["src"]) + channel * int(e["ch_stride"]) + int(e["s"])
    return sources[at:at + int(e["n"])]


def terms32(e, sources, gains, channel, sample_rate):
    """the n terms of event e on one channel, fp32 step by step"""
    n, sf, ef = int(e["n"]), int(e["sf"]), int(e["ef"])
    i = np.arange(n)
    v = np.array(_source(e, sources, channel), F32)
    if sf > 0:
        v[:sf] = v[:sf] * np.sqrt(i[:sf].astype(F32) / F32(sf))
    if ef > 0:
        v[n - ef:] = v[n - ef:] * np.sqrt((n - 1 - i[n - ef:]).astype(F32) / F32(ef))
    if e["flags"] & HANN:
        step, length = F32(1.0) / F32(sample_rate), F32(n) / F32(sample_rate)
        a = TWO_PI_F32 * ((i.astype(F32) * step) / length)
        v = v * (0.5 * (1.0 - np.cos(a.astype(np.float64)))).astype(F32)      # the double cos
    g = gains[int(e["gain_offset"]):int(e["gain_offset"]) + n] if e["gain_offset"] >= 0 else F32(e["gain"])
    return (v * g).astype(F32)


def terms64(e, sources, gains, channel, sample_rate):
    n, sf, ef = int(e["n"]), int(e["sf"]), int(e["ef"])
    i = np.arange(n, dtype=np.float64)
    v = np.array(_source(e, sources, channel), np.float64)
    if sf > 0:
        v[:sf] *= np.sqrt(i[:sf] / sf)
    if ef > 0:
        v[n - ef:] *= np.sqrt((n - 1 - i[n - ef:]) / ef)
    if e["flags"] & HANN:
        v *= 0.5 * (1.0 - np.cos(2.0 * np.pi * i / n))
    g = gains[int(e["gain_offset"]):int(e["gain_offset"]) + n].astype(np.float64) if e["gain_offset"] >= 0 else float(e["gain"])
    return v * g


def _mix(ev, sources, gains, num_channels, frames, sample_rate, dtype, terms, order=None):
    sources = np.ascontiguousarray(sources, F32).reshape(-1)
    gains = None if gains is None else np.ascontiguousarray(gains, F32).reshape(-1)
    out = np.zeros((num_channels, frames), dtype)               # clear_buffer(): +0
    for index in (range(len(ev)) if order is None else order):  # :155-167
        e = ev[index]
        n, o = int(e["n"]), int(e["o"])
        lo, hi = max(o, 0), min(o + n, frames)
        if n <= 0 or lo >= hi:
            continue
        for c in range(min(int(e["channels"]), num_channels)):
            t = terms(e, sources, gains, c, sample_rate)
            out[c, lo:hi] = out[c, lo:hi] + t[lo - o:hi - o]    # one rounding per addition
    return out


def mix32(ev, sources, gains, num_channels, frames, sample_rate, order=None):
    """order: the event indices in the order they are added (None: ascending, the reference's)"""
    return _mix(ev, sources, gains, num_channels, frames, sample_rate, F32, terms32, order)


def mix64(ev, sources, gains, num_channels, frames, sample_rate):
    return _mix(ev, sources, gains, num_channels, frames, sample_rate, np.float64, terms64)


def materialise(ev, sources, gains, sample_rate):
    """the general path's inputs: every grain cut, faded and windowed into a buffer of its own (gain not applied), and the table that
    mixes those buffers: ( events, sources )"""
    sources = np.ascontiguousarray(sources, F32).reshape(-1)
    out_ev, parts, at = ev.copy(), [], 0
    for k, e in enumerate(ev):
        n, ch = int(e["n"]), int(e["channels"])
        plain = e.copy()
        plain["gain_offset"], plain["gain"] = -1, 1.0
        block = np.zeros((max(ch, 0), n), F32)
        for c in range(ch):
            if n > 0:
                block[c] = terms32(plain, sources, None, c, sample_rate)
        parts.append(block.reshape(-1))
        out_ev["src"][k], out_ev["ch_stride"][k], out_ev["src_frames"][k] = at, n, n
        out_ev["s"][k], out_ev["sf"][k], out_ev["ef"][k], out_ev["flags"][k] = 0, 0, 0, 0
        at += block.size
    flat = np.concatenate(parts) if parts else np.zeros(0, F32)
    return out_ev, (flat if flat.size else np.zeros(1, F32))


# ---- the methods' host arithmetic: the tables Audio::mix, texture, granulate and psola hand to the kernel ---------------------------------
def _curve(fn, t):
    """a Function of time on the fp32 times t: a number stays a number per frame, a callable takes the array"""
    return (np.broadcast_to(F32(fn), t.shape) if np.ndim(fn) == 0 and not callable(fn) else np.asarray(fn(t), F32)).astype(F32)


def mix_table(ins, start_times, amplitudes, sample_rate):
    """Audio::mix's list filling (AudioCombination.cpp:111-139) over inputs of one rate.  ins: float32 [ch][n] arrays, or None for a null Audio;
    amplitudes: numbers or callables of fp32 time arrays.  ( events, sources, gains, channels )"""
    count = max(len(ins), len(start_times), len(amplitudes))
    ins = list(ins) + [ins[i % len(ins)] for i in range(len(ins), count)]
    start_times = list(start_times) + [0.0] * (count - len(start_times))
    step = F32(1.0) / F32(sample_rate)
    ev, flat, gains, at = make_events(count), [], [np.zeros(0, F32)], 0
    offsets = {}
    for i, a in enumerate(ins):
        ev["o"][i] = time_to_frame(start_times[i], sample_rate)
        if a is None:
            continue
        a = np.atleast_2d(np.asarray(a, F32))
        if id(a) not in offsets and not any(a is b for b, _ in offsets.values()):
            offsets[id(a)] = (a, at)
            flat.append(a.reshape(-1))
            at += a.size
        ev["src"][i] = offsets[id(a)][1]
        ev["ch_stride"][i] = ev["src_frames"][i] = ev["n"][i] = a.shape[1]
        ev["channels"][i] = a.shape[0]
        if i < len(amplitudes):
            if callable(amplitudes[i]):
                t = ((int(ev["o"][i]) + np.arange(a.shape[1])).astype(F32) * step).astype(F32)       # global time (:138)
                ev["gain_offset"][i] = sum(g.size for g in gains)
                gains.append(_curve(amplitudes[i], t))
            else:
                ev["gain"][i] = amplitudes[i]
    channels = max([int(c) for c in ev["channels"]] + [0])
    return ev, np.concatenate(flat) if flat else np.zeros(1, F32), np.concatenate(gains), channels


def mix_method(ins, start_times=(), amplitudes=(), sample_rate=48000.0, dtype=F32):
    ev, sources, gains, channels = mix_table(ins, start_times, amplitudes, sample_rate)
    return (mix32 if dtype == F32 else mix64)(ev, sources, gains, channels, out_frames(ev), sample_rate)


def join_times(lengths_frames, offsets, sample_rate):
    """Audio::join's start times (:212-218): fp32 running sums of get_length() + offsets[i + 1]"""
    times = [F32(0)]
    for i in range(len(lengths_frames) - 1):
        times.append(F32(F32(times[-1] + F32(lengths_frames[i]) / F32(sample_rate)) + F32(offsets[i + 1])))
    return times


def grain_table(x, sample_rate, event_frames, selection, grain_length, fade, flags=0):
    """granulate's grains (AudioSynthesis.cpp:588-595) for events at event_frames: selection, grain_length and fade are per-frame fp32 arrays, read
    at time_to_frame( frame / sample_rate ); the grain lies there in the output.  x: float32 [ch][N]"""
    x = np.atleast_2d(x)
    at = [time_to_frame(event_time(f, sample_rate), sample_rate) for f in event_frames]
    start = np.array([selection[a] for a in at], F32)
    with np.errstate(all="ignore"):
        end = (start + np.array([grain_length[a] for a in at], F32)).astype(F32)
    fades = np.array([fade[a] for a in at], F32)
    ev = cut_table(x.shape[1], sample_rate, start, end, fades, fades)
    ev["o"] = at
    ev["ch_stride"], ev["src_frames"], ev["channels"], ev["flags"] = x.shape[1], x.shape[1], x.shape[0], flags
    return ev


def granulate_table(x, sample_rate, length, rate, selection, grain_length, fade, flags=0):
    """Audio::granulate with no scatter: rate, selection, grain_length, fade are numbers or callables of fp32 time arrays"""
    frames = time_to_frame(length, sample_rate)
    t = (np.arange(frames).astype(F32) * (F32(1.0) / F32(sample_rate))).astype(F32)
    return grain_table(x, sample_rate, events(frames, sample_rate, _curve(rate, t)), _curve(selection, t), _curve(grain_length, t), _curve(fade, t), flags)


def frequency_envelope(frequencies, t, sample_rate, hop=128):
    """Audio::get_frequency_envelope's function (AudioInformation.cpp:394-406) on fp32 times, in fp32"""
    f = np.asarray(frequencies, F32)
    x = ((np.asarray(t, F32) * F32(sample_rate)).astype(F32) / F32(hop)).astype(F32)
    inside = (x >= 0) & (x < F32(max(f.size - 1, 0))) if f.size else np.zeros(x.shape, bool)
    x1 = np.where(inside, np.floor(x), 0).astype(np.int64)
    if f.size < 2:
        return np.zeros(x.shape, F32)
    y1, y2 = f[x1], f[np.minimum(x1 + 1, f.size - 1)]
    value = (y1 + ((y2 - y1) / F32(1)) * (x - x1.astype(F32))).astype(F32)
    return np.where(inside, value, F32(0)).astype(F32)


def psola_table(x, sample_rate, length, selection, frequencies):
    """Audio::psola without a mod (AudioSynthesis.cpp:611-638) over the per-hop frequencies of get_local_frequencies: the rate is the envelope
    at the selected time, a grain two periods long with 0.05 s fades under the Hann window"""
    sr = F32(sample_rate)
    step = F32(1.0) / sr
    whole = int(np.ceil(F32(length) * sr))                       # :620
    picked_all = _curve(selection, (np.arange(whole).astype(F32) * step).astype(F32))
    frames = time_to_frame(length, sample_rate)
    at = ((np.arange(frames).astype(F32) * step).astype(F32) * sr).astype(F32).astype(np.int64)     # time_to_frame( t ) of the sampling times
    picked = picked_all[np.minimum(at, whole - 1)]
    rate = frequency_envelope(frequencies, picked, sample_rate)
    with np.errstate(all="ignore"):
        lengths = (F32(2.0) / rate).astype(F32)                 # :634
    return grain_table(x, sample_rate, events(frames, sample_rate, rate), picked, lengths, np.full(frames, 0.05, F32), HANN)
