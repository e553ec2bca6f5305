"""Audio silence removal and slicing restated in NumPy from the reference's sources (Audio/AudioTemporal.cpp:10-188, 409-546 over
Audio/AudioCombination.cpp:127-129, 181-221):

  loud_chunks( ... )          the sequential loop of :20-48 exactly as written: three variables of state, one pass over the frames
  fades( ... )                the fades plan of :52-83 in np.float32 arithmetic: the count + 1 fade_ins, the sequential overwrite, the round trips
                              through frame_to_time / time_to_frame, the cuts by cut_frames' rules, the offsets -2 * fade_ins[i]
  remove_silence_table( ... ) those cuts as one event table, placed by join's fp32 running sum and mix's time_to_frame
  edge_cut( ... )             :129-152
  split_frames( ... ), split_lengths_times( ... ), equal_lengths( ... )       :409-461
  rearrange_order( ... )      the Fisher-Yates include/flanhip.h documents, over MT19937
  random_chunks_plan( ... )   :493-533
  reverse( ... )              :174-188
  boundaries_event( ... )     modify_boundaries_frames' one event (:96-114 over mix_in_place)

Event tables are grains_reference.EVENT records; the audio is grains_reference.mix32's ordered fp32 sum."""
import numpy as np

import grains_reference as G

F32 = np.float32
INT_MIN = -2**31


def time_to_frame(t, sr):
    """Frame( time_to_frame( t ) ): the fp32 product truncated"""
    return int(F32(F32(t) * F32(sr)))


def frame_to_time(f, sr):
    return F32(F32(f) / F32(sr))


def noisy(x, level):
    """per frame: some channel's sample is above the level (signed; a NaN never is)"""
    with np.errstate(invalid="ignore"):
        return np.any(np.atleast_2d(x) > F32(level), axis=0)


def loud_chunks(x, level, gap):
    """:20-48 as written.  x: float32 [ch][n].  A list of [ start, end ]"""
    x = np.atleast_2d(np.asarray(x, F32))
    ch, n = x.shape
    level = F32(level)
    noisy_start = INT_MIN
    last_noisy_frame = 0
    in_quiet_sector = True
    chunks = []
    for frame in range(n):
        for channel in range(ch):
            if x[channel, frame] > level:
                last_noisy_frame = frame
                if in_quiet_sector:
                    noisy_start = frame
                    in_quiet_sector = False
                break
        if not in_quiet_sector and frame - last_noisy_frame > gap:
            in_quiet_sector = True
            chunks.append([noisy_start, last_noisy_frame])
    if not in_quiet_sector:
        chunks.append([noisy_start, n])
    return chunks


def summary(x, level, gap):
    where = np.flatnonzero(noisy(x, level))
    count = len(loud_chunks(x, level, gap))
    return [count, int(where[0]) if where.size else -1, int(where[-1]) if where.size else -1, 0]


def fades(num_frames, sr, chunks, fade_in_time):
    """:52-83: ( cuts, fade_ins, offsets ): cuts[i] = ( s, n, sf, ef ) of chunk i by cut_frames' rules"""
    fade_ins = [F32(fade_in_time)] * (len(chunks) + 1)
    for i, (c0, c1) in enumerate(chunks):
        fade_frames_i = time_to_frame(fade_ins[i], sr)                                    # read after iteration i - 1 wrote it
        fade_ins[i] = frame_to_time(c0 if c0 - fade_frames_i < 0 else fade_frames_i, sr)
        fade_ins[i + 1] = frame_to_time(num_frames - c1 if c1 + fade_frames_i >= num_frames else fade_frames_i, sr)
    cuts = []
    for i, (c0, c1) in enumerate(chunks):
        left, right = time_to_frame(fade_ins[i], sr), time_to_frame(fade_ins[i + 1], sr)
        cuts.append(G.cut_frames(num_frames, c0 - left, c1 + right, left, right))
    offsets = [F32(F32(-2) * f) for f in fade_ins]
    return cuts, fade_ins, offsets


def _table(cuts, num_frames, channels):
    ev = G.make_events(len(cuts))
    for i, (s, n, sf, ef) in enumerate(cuts):
        ev["s"][i], ev["n"][i], ev["sf"][i], ev["ef"][i] = s, n, sf, ef
    ev["ch_stride"], ev["src_frames"], ev["channels"] = num_frames, num_frames, channels
    return ev


def join_frames(lengths, offsets, sr):
    """join's start frames (AudioCombination.cpp:212-218 and :127-129) for pieces of the given frame counts"""
    return [time_to_frame(t, sr) for t in G.join_times(lengths, offsets, sr)]


def remove_silence_table(x, sr, level, minimum_gap, fade_in_time):
    """the event table of remove_silence over x itself, or None where nothing is noisy"""
    x = np.atleast_2d(x)
    chunks = loud_chunks(x, level, time_to_frame(minimum_gap, sr))
    if not chunks:
        return None
    cuts, _, offsets = fades(x.shape[1], sr, chunks, fade_in_time)
    ev = _table(cuts, x.shape[1], x.shape[0])
    ev["o"] = join_frames([c[1] for c in cuts], offsets, sr)
    return ev


def chunk_tables(x, sr, level, minimum_gap, fade_in_time):
    """get_loud_chunks: one single-event table per chunk"""
    x = np.atleast_2d(x)
    chunks = loud_chunks(x, level, time_to_frame(minimum_gap, sr))
    if not chunks:
        return []
    cuts, _, _ = fades(x.shape[1], sr, chunks, fade_in_time)
    return [_table([c], x.shape[1], x.shape[0]) for c in cuts]


def render(ev, x, sr, frames=None):
    """the table mixed over x: float32 [ch][frames], or None for what the library calls a null Audio"""
    x = np.atleast_2d(np.asarray(x, F32))
    if ev is None or not np.any(ev["n"] > 0):
        return None
    frames = G.out_frames(ev) if frames is None else frames
    if frames < 1:
        return None
    return G.mix32(ev, x, None, x.shape[0], frames, sr)


def edge_cut(x, sr, level, fade_time):
    """:129-152: the arguments of cut_frames"""
    x = np.atleast_2d(x)
    n = x.shape[1]
    where = np.flatnonzero(noisy(x, level))
    start_frame = int(where[0]) if where.size else n
    end_frame = int(where[-1]) + 1 if where.size else 0
    fade_frames = time_to_frame(fade_time, sr)
    start_fade = start_frame if start_frame - fade_frames < 0 else fade_frames
    end_fade = n - end_frame if end_frame + fade_frames >= n else fade_frames
    return start_frame - fade_frames, end_frame + fade_frames, start_fade, end_fade


def cut_audio(x, sr, start, end, start_fade=0, end_fade=0):
    x = np.atleast_2d(x)
    return render(_table([G.cut_frames(x.shape[1], start, end, start_fade, end_fade)], x.shape[1], x.shape[0]), x, sr)


def split_frames(num_frames, sr, times):
    """:416-429"""
    frames = [0]
    for t in sorted(F32(t) for t in times):
        f = time_to_frame(t, sr)
        if f <= 0:
            continue
        if num_frames <= f:
            break
        frames.append(f)
    frames.append(num_frames)
    return frames


def split_lengths_times(lengths):
    """:445-449: clamped at 0, an fp32 partial_sum"""
    out, acc = [], None
    for v in lengths:
        v = F32(max(F32(v), F32(0)))
        acc = v if acc is None else F32(acc + v)
        out.append(acc)
    return out


def equal_lengths(num_frames, sr, slice_length):
    """:458-459"""
    if slice_length <= 0:
        return []
    return [F32(slice_length)] * int(np.ceil(F32(F32(num_frames) / F32(sr)) / F32(slice_length)))


def split_pieces(x, sr, frames, fade):
    fade_frames = time_to_frame(fade, sr)
    return [cut_audio(x, sr, frames[i], frames[i + 1], fade_frames, fade_frames) for i in range(len(frames) - 1)]


def rearrange_order(count, seed):
    """for i = count - 1 down to 1: swap( order[i], order[g() % ( i + 1 )] ), g = std::mt19937( seed )"""
    g = MT19937(seed)
    order = list(range(count))
    for i in range(count - 1, 0, -1):
        j = g() % (i + 1)
        order[i], order[j] = order[j], order[i]
    return order


class MT19937:
    """std::mt19937( seed )(): the 32-bit Mersenne twister with the standard's seeding"""

    def __init__(self, seed):
        rs = np.random.RandomState()
        key = np.zeros(624, np.uint32)
        key[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            key[i] = (1812433253 * (int(key[i - 1]) ^ (int(key[i - 1]) >> 30)) + i) & 0xFFFFFFFF
        rs.set_state(("MT19937", key, 624))
        self.rs = rs

    def __call__(self):
        return int(self.rs.randint(0, 2**32, dtype=np.uint64))


def random_chunks_loop_frames(sr, length):
    end = F32(F32(length) * F32(sr))
    frames = int(end)
    return frames + 1 if F32(frames) < end else frames


def random_chunks_plan(num_frames, sr, length, chunk_length, fade, seed):
    """:493-533.  chunk_length, fade: callables of an fp32 time, or numbers.  ( cuts, chunk_starts, offsets, o )"""
    cl = chunk_length if callable(chunk_length) else (lambda t: F32(chunk_length))
    fd = fade if callable(fade) else (lambda t: F32(fade))
    starts, acc = [], 1.0
    lowest, longest = frame_to_time(32, sr), F32(F32(num_frames) / F32(sr))
    for f in range(random_chunks_loop_frames(sr, length)):
        if acc >= 1:
            starts.append(f)
            acc = float(np.fmod(acc, 1.0))
        wanted = F32(cl(frame_to_time(f, sr)))
        seconds = float(lowest if wanted < lowest else longest if longest < wanted else wanted)
        acc += 1.0 / seconds / float(F32(sr))
    starts.append(time_to_frame(length, sr))
    fds = [F32(fd(frame_to_time(s, sr))) for s in starts]
    rng = MT19937(seed)
    cuts = []
    for i in range(len(starts) - 1):
        desired = starts[i + 1] - starts[i] + time_to_frame(F32(F32(fds[i] + fds[i + 1]) / F32(2)), sr)
        start = 0 if desired >= num_frames else rng() % (num_frames - desired)
        cuts.append(G.cut_frames(num_frames, start, start + desired, time_to_frame(fds[i], sr), time_to_frame(fds[i + 1], sr)))
    offsets = [F32(-f) for f in fds]
    return cuts, starts[:-1], offsets, join_frames([c[1] for c in cuts], offsets, sr)


def reverse(x):
    return np.ascontiguousarray(np.atleast_2d(x)[:, ::-1])


def boundaries_event(num_frames, sr, start_frame, end_frame):
    """:96-114: ( out_frames, o ) of the one event, or None for a null Audio"""
    out_frames = -start_frame + num_frames + end_frame
    if out_frames <= 0:
        return None
    return out_frames, time_to_frame(F32(-frame_to_time(start_frame, sr)), sr)


def modify_boundaries(x, sr, start_frame, end_frame):
    x = np.atleast_2d(np.asarray(x, F32))
    b = boundaries_event(x.shape[1], sr, start_frame, end_frame)
    if b is None:
        return None
    ev = _table([(0, x.shape[1], 0, 0)], x.shape[1], x.shape[0])
    ev["o"] = b[1]
    return G.mix32(ev, x, None, x.shape[0], b[0], sr)
