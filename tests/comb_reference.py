"""Audio::filter_comb (Audio/AudioFilter.cpp:988-1043) restated in NumPy: the links, the reference's fp32 loop, the same loop in fp64 from the
same fp32 links and coefficients (the "truth"), and the model of the device (flan_amd/csrc/comb.hip): pointer-jumping rounds in fp64, u rounded
to fp32 once, the fp32 output line.  No GPU, no flan_amd.  Also the case table the CPU and the GPU tests share; every expected result is
computed once per process and handed out read-only."""
import functools

import numpy as np

F32, F64 = np.float32, np.float64
SR = 48000.0


def clamp(cutoff, sr):
    """:1009 std::clamp( c, 1.0f, sr / 2.0f ) as two comparisons: a NaN stays"""
    c = np.asarray(cutoff, F32)
    nyquist = F32(sr) / F32(2)
    return np.where(c < F32(1), F32(1), np.where(nyquist < c, nyquist, c)).astype(F32)


def links(n, sr, cutoff):
    """p[n]: the frame u is read at, int32, -1 where the reference reads 0 (:1016-1020, :1031-1032, AudioBuffer.cpp:406-409), in fp32:
    delay = 1 / ( 2 w ), d = delay * sr, t = float( n ) - d, p = (int) t toward zero; a link if 0 <= p < n.  A NaN t: none"""
    w = clamp(np.broadcast_to(np.asarray(cutoff, F32), (n,)), sr)
    frames = np.arange(n, dtype=np.int64)
    with np.errstate(all="ignore"):
        delay = F32(1) / (F32(2) * w)
        d = delay * F32(sr)
        t = frames.astype(F32) - d
    assert t.dtype == F32
    ok = (t > F32(-1)) & (t < F32(2.0 ** 31))
    p = np.where(ok, np.trunc(np.where(ok, t, F32(0))), -1).astype(np.int64)
    return np.where(p < frames, p, -1).astype(np.int32)


def coefficients(n, feedback, wet_dry, invert):
    """( k * f, a, ( 1 - a ) * f ) per frame in fp32 (:1006, :1035, :1038)"""
    f = F32(-1 if invert else 1)
    k = np.broadcast_to(np.asarray(feedback, F32), (n,))
    a = np.broadcast_to(np.asarray(wet_dry, F32), (n,))
    return (k * f).astype(F32), a.astype(F32), ((F32(1) - a) * f).astype(F32)


def _loop(x, p, kf, a, b, dtype):
    ch, n = x.shape
    x, kf, a, b = x.astype(dtype), kf.astype(dtype), a.astype(dtype), b.astype(dtype)
    u, y = np.zeros((ch, n), dtype), np.zeros((ch, n), dtype)
    zero = np.zeros(ch, dtype)
    with np.errstate(all="ignore"):
        for i in range(n):
            um = u[:, p[i]] if p[i] >= 0 else zero
            ui = x[:, i] + kf[i] * um
            u[:, i] = ui
            y[:, i] = a[i] * ui + b[i] * um
    assert u.dtype == dtype and y.dtype == dtype
    return y, u


def comb_fp32(x, sr, cutoff, feedback=0.0, wet_dry=0.5, invert=False):
    """the reference's loop, one fp32 rounding per operation: ( y, u )"""
    x = np.asarray(x, F32)
    return _loop(x, links(x.shape[1], sr, cutoff), *coefficients(x.shape[1], feedback, wet_dry, invert), F32)


def comb_fp64(x, sr, cutoff, feedback=0.0, wet_dry=0.5, invert=False):
    """the truth: the same loop in fp64 from the SAME fp32 links, k * f, a and ( 1 - a ) * f: ( y, u )"""
    x = np.asarray(x, F32)
    return _loop(x, links(x.shape[1], sr, cutoff), *coefficients(x.shape[1], feedback, wet_dry, invert), F64)


def comb_jump(x, sr, cutoff, feedback=0.0, wet_dry=0.5, invert=False):
    """the model of the device: ( y, u in fp32, the rounds that did work ).  A round, for every frame with a live link q = P[n]:
    X[n] += C[n] X[q], C[n] *= C[q], P[n] = P[q], all from the values before the round"""
    x = np.asarray(x, F32)
    n = x.shape[1]
    p = links(n, sr, cutoff)
    kf, a, b = coefficients(n, feedback, wet_dry, invert)
    P, C, X = p.copy(), kf.astype(F64), x.astype(F64)
    rounds = 0
    with np.errstate(all="ignore"):
        while np.any(P >= 0):
            live = P >= 0
            q = np.where(live, P, 0)
            X = np.where(live, X + C * X[:, q], X)
            C = np.where(live, C * C[q], C)
            P = np.where(live, P[q], -1).astype(np.int32)
            rounds += 1
        u = X.astype(F32)
        um = np.where(p >= 0, u[:, np.maximum(p, 0)], F32(0)).astype(F32)
        y = a * u + b * um
    assert y.dtype == F32
    return y, u, rounds


def output_bound(a, b, p, u_truth):
    """5 * 2^-24 * ( | a u[n] | + | ( 1 - a ) u[p] | ) per sample, from the truth: one rounding each of u[n], u[p], 1 - a, the two
    products and the sum, plus second order"""
    um = np.where(p >= 0, u_truth[:, np.maximum(p, 0)], 0.0)
    return 5.0 * 2.0 ** -24 * (np.abs(a.astype(F64) * u_truth) + np.abs(b.astype(F64) * um))


def descendants(p, m):
    """the frames that hang on frame m, m itself included"""
    d = np.zeros(len(p), bool)
    d[m] = True
    for i in range(m + 1, len(p)):
        d[i] = p[i] >= 0 and d[p[i]]
    return d


# ---- the case table: name -> ( frames, channels, cutoff, feedback, wet_dry, invert, input ) ----------------------------------------
# cutoff: c24000 (d = 1: one chain of n, every round is needed), c440 (d = 54.54..., fractional), c1 (no links), sweep (200 -> 8000 Hz
# exponential: links cross), forest (drawn per frame from [1, 24000]), nan (the sweep with a NaN at frame 5000)
# feedback: k0 (the default), k09, k1 (exactly 1.0), kcurve (drawn per frame from [-0.95, 0.95]); wet_dry: a0, a05, a1, acurve
# Which values meet in a case is chosen so that the bounds, which are RELATIVE to the truth's u, have a truth to be relative to: the truth
# is an fp64 loop, exact to about 2^-53 of the terms it sums, and u goes through fp32, whose normal range ends at 2^-126.  So (a) a
# feedback of magnitude exactly 1 meets noise or an impulse, not the sine: its running sums of a periodic input cancel to 1e-15 and
# below, where the truth is rounding noise and 2^-23 | u | asks for more than fp64 holds; (b) an impulse's tail stays normal: 0.9^m
# underflows fp32 after 830 links, so the impulse meets k = 1 on the chain of n and 0.9 only where the links are 55 frames long
CASES = {
    "n1": (1, 1, "c24000", "k09", "a05", False, "noise"),
    "n2": (2, 2, "c24000", "k09", "a05", True, "noise"),
    "n17": (17, 3, "c24000", "kcurve", "acurve", False, "noise"),
    "n4095": (4095, 1, "c24000", "k09", "a0", False, "noise"),
    "n4096": (4096, 2, "c24000", "k1", "a05", False, "noise"),
    "n4097": (4097, 3, "c24000", "k1", "a1", True, "impulse"),
    "chain": (12305, 3, "c24000", "k09", "a05", False, "noise"),
    "chain_k1": (12305, 2, "c24000", "k1", "acurve", True, "noise"),
    "chain_sine": (12305, 2, "c24000", "k09", "a0", True, "sine"),
    "c440": (12305, 3, "c440", "k09", "a05", False, "noise"),
    "c440_k1_impulse": (12305, 1, "c440", "k1", "a0", True, "impulse"),
    "c440_k09_impulse": (12305, 2, "c440", "k09", "acurve", False, "impulse"),
    "c440_default": (12305, 2, "c440", "k0", "a05", False, "sine"),
    "c440_kcurve": (12305, 3, "c440", "kcurve", "a1", False, "noise"),
    "c1_no_links": (12305, 3, "c1", "k09", "acurve", False, "noise"),
    "sweep": (12305, 3, "sweep", "kcurve", "acurve", False, "noise"),
    "sweep_k0": (12305, 2, "sweep", "k0", "acurve", True, "noise"),
    "sweep_k09_sine": (12305, 1, "sweep", "k09", "a05", False, "sine"),
    "forest": (12305, 3, "forest", "kcurve", "acurve", True, "noise"),
    "forest_k1": (12305, 2, "forest", "k1", "a0", False, "noise"),
    "forest_small": (4097, 2, "forest", "k09", "a05", True, "impulse"),
    "nan_cutoff": (12305, 3, "nan", "k09", "a05", False, "noise"),
}
IDS = sorted(CASES)
FEEDBACK = {"k0": 0.0, "k09": 0.9, "k1": 1.0}
WET_DRY = {"a0": 0.0, "a05": 0.5, "a1": 1.0}


def _frozen(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def case(name):
    """the arguments of a case: x float32 [ch][n]; cutoff, feedback and wet_dry each a float or a float32 [n]"""
    n, ch, cutoff, feedback, wet_dry, invert, signal = CASES[name]
    rng = np.random.default_rng(IDS.index(name) + 1)
    frames = np.arange(n)
    if cutoff in ("sweep", "nan"):
        c = (200.0 * (8000.0 / 200.0) ** (frames / max(n - 1, 1))).astype(F32)
        if cutoff == "nan":
            c[5000] = np.nan
    elif cutoff == "forest":
        c = rng.uniform(1.0, 24000.0, n).astype(F32)
    else:
        c = float(cutoff[1:])
    k = rng.uniform(-0.95, 0.95, n).astype(F32) if feedback == "kcurve" else FEEDBACK[feedback]
    a = rng.uniform(0.0, 1.0, n).astype(F32) if wet_dry == "acurve" else WET_DRY[wet_dry]
    if signal == "noise":
        x = rng.uniform(-1.0, 1.0, (ch, n)).astype(F32)
    elif signal == "impulse":
        x = np.zeros((ch, n), F32)
        x[:, 0] = [1.0, -0.5, 0.25][:ch]
    else:
        x = np.stack([np.sin(2 * np.pi * 440.0 * frames / SR + c_) for c_ in range(ch)]).astype(F32)
    return {"name": name, "x": _frozen(x), "sr": SR, "cutoff": _frozen(c), "feedback": _frozen(k), "wet_dry": _frozen(a), "invert": invert}


def args(c):
    return c["x"], c["sr"], c["cutoff"], c["feedback"], c["wet_dry"], c["invert"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """p, kf, a, b; y32 / u32 (the fp32 loop), y64 / u64 (the truth), y / u / rounds (the model); bound (on the output)"""
    c = case(name)
    n = c["x"].shape[1]
    p = links(n, c["sr"], c["cutoff"])
    kf, a, b = coefficients(n, c["feedback"], c["wet_dry"], c["invert"])
    y32, u32 = comb_fp32(*args(c))
    y64, u64 = comb_fp64(*args(c))
    y, u, rounds = comb_jump(*args(c))
    e = {"p": p, "kf": kf, "a": a, "b": b, "y32": y32, "u32": u32, "y64": y64, "u64": u64, "y": y, "u": u, "rounds": rounds,
         "bound": output_bound(a, b, p, u64)}
    return {key: _frozen(v) for key, v in e.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F32 and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
