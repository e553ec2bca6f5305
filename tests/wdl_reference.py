"""WDL_Resampler's windowed-sinc mode (WDL/resample.cpp, SetMode( true, 0, true, taps )) restated in Python as far as it does not depend on
who feeds it: the choice of table, the table, the stream and the evaluation of a block's output samples, in the reference's own operation
order.  tests/repitch_reference.py uses it at 64 taps, tests/spatial_reference.py at 32.  DESIGN.md 4.13.

The table runs in scalar Python (math.sin / math.cos: the libm the reference calls); the tap sums are numpy fp32 products accumulated in
fp64 in tap order."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
OVERSIZE = 32                                           # m_sincoversize (SetMode's default): the slices of a table unless the rates are "ideal"


def table_shape(rate_in, rate_out, ratio):
    """BuildLowPass's first half (:1095-1141): ( filtpos, oversize, ideal ); it does not depend on the tap count"""
    filtpos = 1.0 / (ratio * 1.03) if ratio > 1.0 else 1.0                  # :1327-1328
    want, ideal_interp = OVERSIZE, 0
    if ratio < 1.0:
        drat = rate_out / rate_in
        irat = int(drat + 0.5)
        if irat > 1 and irat == drat:
            ideal_interp = irat
    else:
        irat = int(ratio + 0.5)
        if ratio == irat:
            ideal_interp = 1
    if not ideal_interp and rate_in < 2147483648.0 and rate_out < 2147483648.0:
        in1, out1 = int(rate_in), int(rate_out)
        if out1 > 0 and in1 > 0 and rate_in == in1 and rate_out == out1:
            min_cd = max(out1 // (2 * want), 1)
            n1, n2 = out1, in1
            while n2 >= min_cd:
                n1, n2 = n2, n1 % n2
            if not n2:
                ideal_interp = out1 // n1
    if 0 < ideal_interp <= want * 2:
        want = ideal_interp
    return filtpos, want, ideal_interp == want


def window(x_frac, taps, cos=math.cos):
    """the Blackman-Harris factor of :1185 at table position xfrac (slice / oversize + tap); cos: numpy's for an array of positions"""
    wp = (2.0 * math.pi / taps) * x_frac
    return 0.35875 - 0.48829 * cos(wp) + 0.14128 * cos(2 * wp) - 0.01168 * cos(3 * wp)


def half_table(filtpos, oversize, taps):
    """BuildLowPass's loop (:1157-1190): ( the fp64 values of the table's first half, filtpower )"""
    half = taps // 2
    dsincpos = math.pi * filtpos
    vals, power = [], 0.0
    for sl in range(oversize // 2 + 1):
        frac = sl / float(oversize)
        count = taps if (sl < oversize // 2 or oversize & 1) else half
        for x in range(count):
            if sl == 0 and x == half:
                vals.append(1.0)
                continue
            xfrac = frac + x
            sincpos = dsincpos * (xfrac - half)
            val = window(xfrac, taps) * math.sin(sincpos) / sincpos
            power += val * 2 if sl else val
            vals.append(val)
    assert len(vals) == taps * (oversize + 1) // 2
    return vals, power


_tables = {}


def table(filtpos, oversize, taps):
    """BuildLowPass's second half (:1157-1202): float32 [(oversize + 1) * taps]"""
    key = (filtpos, oversize, taps)
    if key not in _tables:
        vals, power = half_table(filtpos, oversize, taps)
        first = np.array(vals, np.float64).astype(F32)
        first = (first.astype(np.float64) * (oversize / (power + 1.0))).astype(F32)         # :1193
        _tables[key] = np.concatenate([first, first[::-1]])
    return _tables[key]


def stream_window(x, prelude, start, length):
    """float32 [...][length] of the stream (prelude zeros, x [...][n], zeros) from index `start`"""
    n = x.shape[-1]
    out = np.zeros(x.shape[:-1] + (length,), F32)
    a, b = max(start - prelude, 0), min(start - prelude + length, n)
    if b > a:
        out[..., a - (start - prelude):b - (start - prelude)] = x[..., a:b]
    return out


def tap_sums(coef, taps):
    """per output sample, the sum over the taps of float( coef * tap ) added into fp64 in tap order; coef [m][taps], taps [...][m][taps] ->
    float64 [...][m]"""
    prod = (coef * taps).astype(F32).astype(np.float64)                     # fp32 products, each rounded
    s = np.zeros(prod.shape[:-1], np.float64)
    for i in range(prod.shape[-1]):
        s = s + prod[..., i]
    return s


def _fma(j, ratio, fracpos):
    """fma( j, ratio, fracpos ) with one rounding, from exact rational arithmetic"""
    return float(Fraction(j) * Fraction(ratio) + Fraction(fracpos))


def positions(fracpos, ratio, m, position):
    """srcpos of a block's first m output samples, float64 [m].  position: "chain" forms them by repeated += ratio like the reference, "fma"
    as fracpos + j * ratio with one rounding like the device kernel"""
    if position == "fma":
        return np.array([_fma(j, ratio, fracpos) for j in range(m)], np.float64)
    srcpos = np.empty(m, np.float64)
    p = fracpos
    for j in range(m):
        srcpos[j] = p
        p += ratio
    return srcpos


def samples(srcpos, buf, tab, ideal):
    """The output samples at positions srcpos (relative to the first sample of buf): SincSample1N (:184-200) where the table is ideal,
    else SincSample1 (:160-182).  buf float32 [...][length], tab [oversize + 1][taps] -> float32 [...][m]"""
    oversize, size = tab.shape[0] - 1, tab.shape[1]
    ipos = srcpos.astype(np.int64)                                          # truncation: srcpos >= 0
    frac = srcpos - ipos
    taps = buf[..., ipos[:, None] + np.arange(size)[None, :]]               # [...][m][taps]
    if ideal:
        ifpos = (frac * oversize + 0.5).astype(np.int64)
        return tap_sums(tab[oversize - ifpos], taps).astype(F32)
    fr = frac * oversize
    ifpos = fr.astype(np.int64)
    fr = fr - ifpos
    s1 = tap_sums(tab[oversize - ifpos - 1], taps)
    s2 = tap_sums(tab[oversize - ifpos], taps)
    return (s1 * fr + s2 * (1.0 - fr)).astype(F32)
