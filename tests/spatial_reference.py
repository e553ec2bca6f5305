"""Audio/AudioSpatial.cpp restated in Python on numpy: Audio::stereo_spatialize (:88-281) -- the speed limiter, head_ild, falloff and
head_itd over WDL_Resampler in feed mode (WDL/resample.cpp) --, pan (:9-45), and the channel plumbing under them (convert_to_stereo /
convert_to_mono, Audio/AudioConversions.cpp:58-104; combine_channels, Audio/AudioChannels.cpp).  DESIGN.md 4.20.

Everything runs in the reference's own types and operation order.  The limiter and the plan run in scalar Python; cosf / atan2f are libm's
through ctypes where it can be loaded (numpy's own otherwise); the resampler itself (the table and the tap sums) is tests/wdl_reference.py's
at 32 taps.  The 500 Hz low-pass is tests/filter_reference.py's."""
import ctypes
import ctypes.util
import math
import os

import numpy as np

import filter_reference as fr
import wdl_reference as W
from repitch_reference import errors                              # noqa: F401
from wdl_reference import table_shape, tap_sums, _fma             # noqa: F401  (this module's names too)

F32, F64 = np.float32, np.float64
G = 32                                                  # granularity_frames (:137)
TAPS, OVERSIZE = 32, 32                                 # SetMode( true, 0, true, 32 ): 32 taps, 32 slices unless the rates are "ideal"
PRELUDE = TAPS // 2 - 1
SOUND = F32(343)                                        # sound_mps (:7)
PI = np.arccos(F32(-1))                                 # defines.h:44-45
PI2 = F32(PI * F32(2))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_made", "wdl_spatial.npz")
LEFT, RIGHT = True, False


def _libm():
    try:
        m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        m.cosf.restype = m.atan2f.restype = ctypes.c_float
        m.cosf.argtypes = [ctypes.c_float]
        m.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
        return m
    except OSError:
        return None


_M = _libm()


def cosf(a):
    a = np.asarray(a, F32)
    if _M is None:
        return np.cos(a).astype(F32)
    return np.array([_M.cosf(float(v)) for v in a.reshape(-1)], F32).reshape(a.shape)


def atan2f(y, x):
    y, x = np.broadcast_arrays(np.asarray(y, F32), np.asarray(x, F32))
    if _M is None:
        return np.arctan2(y, x).astype(F32)
    return np.array([_M.atan2f(float(a), float(b)) for a, b in zip(y.reshape(-1), x.reshape(-1))], F32).reshape(y.shape)


# ---- positions ------------------------------------------------------------------------------------------------------------------------
def limit_positions(positions, speed_limit, sr):
    """:235-257.  positions: float32 [n][2], what the Function returns per frame; speed_limit: a float or float32 [n].  Returns float64
    [n][2].  The movement's length is a Meter (a float), the step is fp64."""
    ps = np.asarray(positions, F32).astype(F64).copy()
    n = ps.shape[0]
    limit = np.broadcast_to(np.asarray(speed_limit, F32), (n,))
    top = F32(SOUND - F32(1))
    for f in range(1, n):
        mx, my = ps[f, 0] - ps[f - 1, 0], ps[f, 1] - ps[f - 1, 1]
        mag = F32(math.sqrt(mx * mx + my * my))
        c = F32(min(max(limit[f], F32(0)), top) / F32(sr))                  # std::clamp, then meters per frame
        if mag > c:
            ps[f, 0] = ps[f - 1, 0] + mx / float(mag) * float(c)
            ps[f, 1] = ps[f - 1, 1] + my / float(mag) * float(c)
    return ps


def limit_positions_direct(positions, speed_limit, sr):
    """the same recurrence written out once more in plain fp64 Python, for the limiter's own test"""
    out = [(float(F32(positions[0][0])), float(F32(positions[0][1])))]
    lim = np.broadcast_to(np.asarray(speed_limit, F32), (len(positions),))
    for f in range(1, len(positions)):
        x, y = float(F32(positions[f][0])), float(F32(positions[f][1]))
        px, py = out[-1]
        dx, dy = x - px, y - py
        mag = float(F32(math.sqrt(dx * dx + dy * dy)))
        c = float(F32(F32(min(max(float(lim[f]), 0.0), 342.0)) / F32(sr)))
        out.append((px + dx / mag * c, py + dy / mag * c) if mag > c else (x, y))
    return np.array(out, F64)


def relative(ps, head_width, left):
    """:261-263: positions minus the ear's, ( 0, +- head_width / 2.0f ), in fp64"""
    ear_y = float(F32((F32(1) if left else F32(-1)) * F32(head_width)) / F32(2))
    rel = np.array(ps, F64, copy=True).reshape(-1, 2)
    rel[:, 1] = rel[:, 1] - ear_y
    return rel


def mag(v):
    v = np.asarray(v, F64)
    return np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])


def read_index(n, sr):
    """the frame whose weight and distance frame f reads: int( ( f * ( 1.0f / sr ) ) * sr ) in fp32 (FunctionSample.h:130-133, :109)"""
    f = np.arange(n, dtype=F32)
    t = (f * F32(F32(1) / F32(sr))).astype(F32)
    return np.clip((t * F32(sr)).astype(F32).astype(np.int64), 0, max(n - 1, 0))


def quirk_frames(n, sr):
    """how many frames read another frame's geometry than their own"""
    return int(np.count_nonzero(read_index(n, sr) != np.arange(n)))


def ear(x, lp, sr, ps, head_width, left):
    """head_ild (:116-131) and falloff (:104-114) of one ear.  x, lp: float32 [n]; ps: float64 [n][2] (after the limiter) or a pair."""
    x, lp = np.asarray(x, F32), np.asarray(lp, F32)
    n = x.size
    rel = relative(np.broadcast_to(np.asarray(ps, F64).reshape(-1, 2), (n, 2)), head_width, left)
    direct = F32(F32(F32(75.0 if left else -75.0) * PI2) / F32(360))
    angle = (atan2f(rel[:, 1].astype(F32), rel[:, 0].astype(F32)) - direct).astype(F32)
    mix = (F32(0.5) + (F32(0.5) * cosf(angle)).astype(F32)).astype(F32)
    gain = (F32(1) / (mag(rel).astype(F32) + F32(0.00001)).astype(F32)).astype(F32)
    q = read_index(n, sr)
    mix, gain = mix[q], gain[q]
    blended = ((lp * (F32(1) - mix).astype(F32)).astype(F32) + (x * mix).astype(F32)).astype(F32)
    return (blended * gain).astype(F32)


# ---- head_itd ---------------------------------------------------------------------------------------------------------------------------
def chunk_count(n):
    return (n + G - 1) // G


def itd_out_frames(n, sr, dist):
    """:159-186 from the distances at frames 0, 32, ...: ( output length, stretches ), with the reference's float / double mix"""
    dist = np.asarray(dist, F64)
    assert dist.size == chunk_count(n)
    sr32 = F32(sr)
    stretches = np.empty(dist.size, F64)
    longest = F32(0)
    previous = float(dist[0])
    stretches[0] = 1.0 / (1.0 - 0.0 / G / float(SOUND) * float(sr32))
    for k in range(1, dist.size):
        current = float(dist[k])
        change = current - previous
        previous = current
        stretches[k] = 1.0 / (1.0 - change / G / float(SOUND) * float(sr32))
        receive = F32(float(F32(F32(k * G + G) / sr32)) + current / float(SOUND))
        if longest < receive:
            longest = receive
    return int(math.ceil(float(F32(longest * sr32)))), stretches


def itd_plan(n, sr, stretches):
    """The block loop (:194-218 with ResamplePrepare in feed mode, WDL/resample.cpp:1218-1265, and ResampleOut's loop and hand-over,
    :1295, :1339-1361, :1558-1566) in fp64, with the reference's chain of srcpos += ratio.  One dict per block: offset (stream index of the
    buffer's first sample; the stream: 15 zeros, the input, zeros to the next multiple of 32), fracpos, ratio, filtpos, oversize, ideal,
    first_out, count, buffered.  It asserts the invariants of DESIGN.md 4.20 on the way."""
    stretches = np.asarray(stretches, F64)
    assert stretches.size == chunk_count(n)
    rate_in = max(float(F32(sr)), 1.0)
    blocks = []
    fracpos, S, offset, out_frame, last_ratio = 0.0, 0, 0, 0, 0.0
    for b, stretch in enumerate(stretches.tolist()):
        rate_out = max(float(F32(sr)) * stretch, 1.0)
        ratio = rate_in / rate_out
        if S < PRELUDE:                                                     # :1226-1237
            assert b == 0, "the prelude is written once: S never drops below it again"
            S = PRELUDE
        else:
            assert 34 - math.ceil(last_ratio) <= S <= 34, "S between blocks: at least 34 - ceil( ratio ), at most 34"
        S += G                                                              # feed mode: 32 frames go in, whatever the rate
        assert offset + S == PRELUDE + G * (b + 1), "the buffer is a window of one continuous stream"
        filtpos, oversize, ideal = table_shape(rate_in, rate_out, ratio)
        ns = int(math.ceil(G * stretch))                                    # :210
        limit = S - TAPS - 1                                                # ipos >= filtlen - 1 ends the block (:1343)
        srcpos, count = fracpos, 0
        while ns and int(srcpos) < limit:
            ns -= 1
            srcpos += ratio
            count += 1
        if b == 0:
            assert limit == 14, "the first block delivers outputs for srcpos < 14 only"
        blocks.append(dict(offset=offset, fracpos=fracpos, ratio=ratio, filtpos=filtpos, oversize=oversize, ideal=ideal,
                           first_out=out_frame, count=count, buffered=S))
        isrcpos = min(int(srcpos), S)                                       # :1558-1560
        fracpos = srcpos - isrcpos
        if ideal:
            fracpos = math.floor(oversize * fracpos + 0.5) / oversize       # :1562-1563
        S -= isrcpos
        offset += isrcpos
        out_frame += count
        last_ratio = ratio
    return blocks


def window(x_frac):
    return W.window(x_frac, TAPS)


def table(filtpos, oversize):
    """BuildLowPass's second half (:1157-1202) at 32 taps: float32 [(oversize + 1) * 32]"""
    return W.table(filtpos, oversize, TAPS)


def stream_window(x, start, length):
    """float32 [length] of the stream (15 zeros, x, zeros) from index `start`"""
    return W.stream_window(x, PRELUDE, start, length)


def itd(x, sr, stretches, nout, position="chain", plan=None):
    """head_itd for a moving source: float32 [nout].  position: "chain" forms srcpos by repeated += ratio like the reference, "fma" as
    fracpos + j * ratio with one rounding like the device kernel (the block hand-over is the chain's in both)."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    out = np.zeros(nout, F32)
    for b in (plan if plan is not None else itd_plan(x.size, sr, stretches)):
        ratio, oversize = b["ratio"], b["oversize"]
        m = min(b["count"], nout - b["first_out"])                          # :213-215
        if m <= 0:
            continue
        srcpos = W.positions(b["fracpos"], ratio, m, position)
        ipos = srcpos.astype(np.int64)
        assert int(ipos[-1]) + TAPS + 1 < b["buffered"], "a window ends at least two samples before the buffer's end"
        buf = stream_window(x, b["offset"], b["buffered"])
        out[b["first_out"]:b["first_out"] + m] = W.samples(srcpos, buf, table(b["filtpos"], oversize).reshape(oversize + 1, TAPS), b["ideal"])
    return out


def constant_delay(x, sr, dist):
    """head_itd for a source that stands still (:139-153): ( delay in frames as a float, output ).  dist: the fp64 distance"""
    x = np.asarray(x, F32).reshape(-1)
    delay = F32(F32(F32(dist) / SOUND) * F32(sr))
    out = np.zeros(int(F32(F32(x.size) + delay)), F32)
    at = (np.arange(x.size, dtype=F32) + delay).astype(F32).astype(np.int64)
    ok = at < out.size
    out[at[ok]] = x[ok]                                                     # (numpy keeps the last of equal indices, like the loop)
    return delay, out


def lowpass500(x, sr, run=None):
    """filter_1pole_lowpass( 500, 1 ) of a mono row; run: the device's scan model instead of the sequential loop"""
    return fr.filter_1pole(np.asarray(x, F32).reshape(1, -1), sr, 500.0, fr.BUTTERWORTH_LOW, 1, run=run)[0]


def stereo_spatialize(x, sr, positions, head_width=0.18, speed_limit=np.finfo(F32).max, lp=None, position="fma"):
    """The whole method: float32 [2][frames of the longer ear], or None where the reference makes a zero-frame Audio (a moving source
    and n <= 32).  positions: float32 [n][2] (what a callable returns per frame) or a pair (a constant Function)."""
    x = np.ascontiguousarray(x, F32).reshape(-1)
    n = x.size
    lp = lowpass500(x, sr) if lp is None else np.asarray(lp, F32)
    constant = np.ndim(positions) == 1
    ps = np.asarray(positions, F32).astype(F64) if constant else limit_positions(positions, speed_limit, sr)
    ears = []
    for left in (LEFT, RIGHT):
        shaped = ear(x, lp, sr, ps, head_width, left)
        rel = relative(ps, head_width, left)
        if constant:
            ears.append(constant_delay(shaped, sr, float(mag(rel)[0]))[1])
        else:
            nout, stretches = itd_out_frames(n, sr, mag(rel[::G]))
            ears.append(itd(shaped, sr, stretches, nout, position))
    if max(e.size for e in ears) == 0:
        return None
    return combine(ears)


# ---- pan, the conversions, combine --------------------------------------------------------------------------------------------------------
def sine2(x):
    """Interpolator::sine2 (Utility/Interpolator.cpp:85-91): pi / 4.0f * x in fp32, the DOUBLE sin of it, times the fp32 sqrt( 2 )
    promoted to double, rounded to fp32 once"""
    x = np.asarray(x, F32)
    arg = (F32(PI / F32(4)) * x).astype(F32).astype(F64)
    return (float(np.sqrt(F32(2))) * np.array([math.sin(v) for v in arg.reshape(-1)], F64).reshape(arg.shape)).astype(F32)


def pan(x, amount):
    """Audio::pan_in_place (:21-40): x float32 [2][n], amount a float or [n]"""
    x = np.asarray(x, F32)
    p = (np.broadcast_to(np.asarray(amount, F32), (x.shape[1],)) / F32(2) + F32(0.5)).astype(F32)
    return np.stack([(x[0] * sine2(p)).astype(F32), (x[1] * sine2((F32(1) - p).astype(F32))).astype(F32)])


def to_stereo(x):
    x = np.asarray(x, F32).reshape(-1)
    half = (x / np.sqrt(F32(2))).astype(F32)
    return np.stack([half, half])


def to_mono(x):
    x = np.asarray(x, F32)
    acc = np.zeros(x.shape[1], F32)
    for row in x:
        acc = (acc + row).astype(F32)
    return (acc / F32(x.shape[0])).astype(F32)


def combine(rows):
    """combine_channels of mono rows: the longest one's length, zeros behind the shorter ones"""
    rows = [np.atleast_2d(np.asarray(r, F32)) for r in rows]
    n = max(r.shape[1] for r in rows)
    out = np.zeros((sum(r.shape[0] for r in rows), n), F32)
    at = 0
    for r in rows:
        out[at:at + r.shape[0], :r.shape[1]] = r
        at += r.shape[0]
    return out


def mid_side(x):
    x = np.asarray(x, F32)
    s = np.sqrt(F32(2))
    return np.stack([((x[0] + x[1]).astype(F32) / s).astype(F32), ((x[0] - x[1]).astype(F32) / s).astype(F32)])


# ---- the reference-made fixture -----------------------------------------------------------------------------------------------------------
def load_cases():
    """the fixture as a list of dicts: name, x, sr, dist, stretches, out, delivered, out_frames"""
    z = np.load(GOLDEN)
    cases = []
    for k, name in enumerate(z["names"]):
        sr, nout, blocks = z["meta_%d" % k]
        cases.append(dict(name=str(name), x=z["x_%d" % k], sr=float(sr), dist=z["dist_%d" % k], stretches=z["stretches_%d" % k],
                          out=z["out_%d" % k], delivered=z["delivered_%d" % k], out_frames=int(nout), blocks=int(blocks)))
    return cases
