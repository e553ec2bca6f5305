"""Audio::repitch (Audio/AudioTemporal.cpp:236-299 over WDL_Resampler, WDL/resample.cpp) restated in Python: the block plan in the
reference's own operation order, in scalar Python, around the resampler itself (the low-pass table and the tap sums:
tests/wdl_reference.py, at 64 taps).  DESIGN.md 4.13.

Also an fp64 "smooth truth" for constant factors: the same windowed sinc evaluated at the exact fractional position, all in fp64."""
import math
import os

import numpy as np

import wdl_reference as W
from wdl_reference import table_shape, stream_window, tap_sums, _fma     # noqa: F401  (this module's names too)

F32 = np.float32
SINC, LINEAR, UNINTERPOLATED = 0, 1, 2
SINC_SIZE, SINC_OVERSIZE = 64, 32                       # SetMode( true, 0, true, 64 ): 64 taps, 32 slices unless the rates are "ideal"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_made", "wdl_repitch.npz")
GOLDEN_RUNS = os.path.join(os.path.dirname(GOLDEN), "wdl_repitch_runs.npz")       # the cases that hold the run planner


def invert(factors):
    """:246-249 in fp32: clamp( 1.0f / v, 1.0f / 1000.0f, 1000.0f )"""
    with np.errstate(divide="ignore"):
        inv = F32(1.0) / np.asarray(factors, F32)
    return np.clip(inv, F32(1.0) / F32(1000.0), F32(1000.0)).astype(F32)


def granularity_frames(granularity_seconds, sr):
    return max(int(F32(granularity_seconds) * F32(sr)), 1)                 # :241-242


def factor_count(n, g):
    return int(np.ceil(F32(n) / F32(g)))                                    # :245


def out_frames(inv, g):
    """:252: FunctionSample<float>::accumulate() of a vector is a sequential fp32 sum; the product and the ceil are fp32 too"""
    s = F32(0.0)
    for v in np.asarray(inv, F32):
        s = F32(s + v)
    return int(np.ceil(F32(s * F32(g))))


def rates(sr, inv):
    """SetRates (:1080-1090) as Audio::repitch calls it: ( rate in, rate out, ratio ), both rates at least 1"""
    rate_in = max(float(F32(sr)), 1.0)
    rate_out = max(float(F32(sr)) * float(F32(inv)), 1.0)
    return rate_in, rate_out, rate_in / rate_out


def plan(n, sr, inv, g, quality=SINC):
    """The block loop (:267-296 with ResamplePrepare :1218-1265 and ResampleOut's state hand-over :1313, :1558-1566) in fp64, with the
    reference's chain of srcpos += ratio additions.  One dict per block:
        offset     stream index of the buffer's first sample (the stream: `prelude` zeros, the input, zeros)
        fracpos    srcpos at the block's first output sample, relative to `offset`
        ratio, filtpos, oversize, ideal, first_out, wanted
    It asserts what the arithmetic promises: every block delivers all g samples, S never drops below the prelude again, and the buffer
    is a window of one continuous stream."""
    inv = np.asarray(inv, F32)
    fsize = SINC_SIZE if quality == SINC else 0
    prelude = fsize // 2 - 1 if fsize else 0
    blocks = []
    fracpos, S, in_frame, out_frame, offset, first = 0.0, 0, 0, 0, 0, True
    while in_frame < n:
        index = int(np.floor(F32(in_frame) / F32(g)))                       # :271, the fp32 quotient
        assert index < inv.size, "count is smaller than the loop needs"
        rate_in, rate_out, ratio = rates(sr, inv[index])
        if fsize // 2 > 1 and S < fsize // 2 - 1:                           # :1226-1237
            assert first, "the prelude is written once: S never drops below it again"
            S = fsize // 2 - 1
        first = False
        wanted = max(int(ratio * g) + 4 + fsize - S, 0)                     # :1241-1244
        S += wanted                                                         # :1295
        assert offset + S == prelude + in_frame + wanted, "the buffer is a window of one continuous stream"
        if fsize:
            filtpos, oversize, ideal = table_shape(rate_in, rate_out, ratio)
            limit = S - fsize - 1                                           # ipos >= filtlen - 1 ends the block early (:1343)
        else:
            filtpos, oversize, ideal = 1.0, 1, False
            limit = S                                                       # :1425
        blocks.append(dict(offset=offset, fracpos=fracpos, ratio=ratio, filtpos=filtpos, oversize=oversize, ideal=ideal,
                           first_out=out_frame, wanted=wanted))
        srcpos = fracpos
        for _ in range(g):
            assert int(srcpos) < limit, "every block delivers all g samples"
            srcpos += ratio
        isrcpos = min(int(srcpos), S)                                       # :1558-1560
        fracpos = srcpos - isrcpos
        if fsize and ideal:
            fracpos = math.floor(oversize * fracpos + 0.5) / oversize       # :1562-1563
        S -= isrcpos
        offset += isrcpos
        in_frame += wanted
        out_frame += g
    return blocks


def window(x_frac):
    return W.window(x_frac, SINC_SIZE)


def table(filtpos, oversize):
    """BuildLowPass's second half (:1157-1202): float32 [(oversize + 1) * 64]"""
    return W.table(filtpos, oversize, SINC_SIZE)


def repitch(x, sr, inv, g, quality=SINC, position="chain"):
    """The whole method: float32 [ch][out_frames].  position: "chain" forms srcpos by repeated += ratio like the reference, "fma"
    as fracpos + j * ratio with one rounding like the device kernel (the block hand-over is the chain's in both)."""
    x = np.ascontiguousarray(x, F32)
    ch, n = x.shape
    nout = out_frames(inv, g)
    out = np.zeros((ch, nout), F32)
    fsize = SINC_SIZE if quality == SINC else 0
    prelude = fsize // 2 - 1 if fsize else 0
    for b in plan(n, sr, inv, g, quality):
        ratio, oversize = b["ratio"], b["oversize"]
        m = min(g, nout - b["first_out"])
        if m <= 0:
            continue
        srcpos = W.positions(b["fracpos"], ratio, m, position)
        ipos = srcpos.astype(np.int64)                                     # truncation: srcpos >= 0
        buf = stream_window(x, prelude, b["offset"], int(ipos[-1]) + SINC_SIZE + 1)
        dst = out[:, b["first_out"]:b["first_out"] + m]
        if not fsize:
            dst[:] = buf[:, ipos]
            continue
        dst[:] = W.samples(srcpos, buf, table(b["filtpos"], oversize).reshape(oversize + 1, SINC_SIZE), b["ideal"])
    return out


def smooth_truth(x, sr, factor, nout):
    """fp64 truth for a constant factor: output sample t is the Blackman-Harris windowed sinc (64 taps, cut-off filtpos, gain
    normalised like the table's) evaluated at the exact position t * ratio of the stream, no table, no slices.  float64 [ch][nout]"""
    x = np.asarray(x, np.float64)
    ch, n = x.shape
    inv = invert([factor])[0]
    rate_in, rate_out, ratio = rates(sr, inv)
    filtpos = table_shape(rate_in, rate_out, ratio)[0]
    half = SINC_SIZE // 2
    prelude = half - 1
    padded = np.zeros((ch, prelude + n + int(nout * ratio) + 2 * SINC_SIZE + 8))
    padded[:, prelude:prelude + n] = x
    t = np.arange(nout, dtype=np.float64) * ratio
    ipos = np.floor(t).astype(np.int64)
    frac = t - ipos
    taps = np.arange(SINC_SIZE, dtype=np.float64)
    # slice s of the table holds xfrac = s / oversize + tap and is read at s = oversize - ifpos: the continuous form is tap + 1 - frac
    xfrac = taps[None, :] + 1.0 - frac[:, None]
    arg = np.pi * filtpos * (xfrac - half)
    coef = W.window(xfrac, SINC_SIZE, np.cos) * np.sinc(arg / np.pi)
    coef *= filtpos_gain(filtpos)
    idx = ipos[:, None] + taps[None, :].astype(np.int64)
    out = np.empty((ch, nout))
    for c in range(ch):
        out[c] = np.sum(coef * padded[c][idx], axis=1)
    return out


def filtpos_gain(filtpos, oversize=SINC_OVERSIZE):
    """the table's normalisation oversize / ( filtpower + 1 ) (:1193), from the fp64 table values"""
    return oversize / (W.half_table(filtpos, oversize, SINC_SIZE)[1] + 1.0)


def errors(y, ref):
    """( relative rms error, max abs error / max |ref| )"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    d = y - ref
    scale = np.max(np.abs(ref)) if ref.size else 0.0
    if scale == 0.0:
        return (0.0, 0.0) if not np.any(d) else (np.inf, np.inf)
    return float(np.sqrt(np.sum(d * d) / np.sum(ref * ref))), float(np.max(np.abs(d)) / scale)


def random_case(seed):
    """the random shapes the planner tests and the device tests share: ( x float32 [ch][n], sr, inv, g, quality )"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 5001))
    ch = int(rng.integers(1, 4))
    g = int(rng.choice([1, 7, 48, 100, 480, 6000])) if n <= 1000 else int(rng.choice([48, 100, 480, 6000]))
    count = factor_count(n, g)
    kind = int(rng.integers(0, 4))
    t = np.arange(count) / max(count - 1, 1)
    if kind == 0:
        v = np.full(count, rng.choice([0.25, 0.5, 0.75, 1.0, 1.25, 2.0, 3.0, 0.9, 1.7]))
    elif kind == 1:
        lo, hi = sorted(rng.uniform(0.3, 3.0, 2))
        v = lo + (hi - lo) * t
    elif kind == 2:
        v = 1.0 + 0.6 * np.sin(2 * np.pi * rng.uniform(0.5, 4.0) * t)
    else:
        v = rng.choice([0.5, 1.0, 1.5, 2.0], count)
    quality = UNINTERPOLATED if seed % 5 == 4 else SINC
    x = (0.5 * rng.standard_normal((ch, n))).astype(F32)
    return x, 48000.0, invert(v.astype(F32)), g, quality


def load_cases(path=GOLDEN):
    """a reference-made fixture as a list of dicts: name, x, inv, sr, g, quality, out, wanted, delivered"""
    z = np.load(path)
    cases = []
    for k, name in enumerate(z["names"]):
        sr, g, quality, nout, blocks = z["meta_%d" % k]
        cases.append(dict(name=str(name), x=z["x_%d" % k], inv=z["inv_%d" % k], sr=float(sr), g=int(g), quality=int(quality),
                          out=z["out_%d" % k], wanted=z["wanted_%d" % k], delivered=z["delivered_%d" % k], out_frames=int(nout), blocks=int(blocks)))
    return cases
