"""Audio::filter_1pole_multinotch (Audio/AudioFilter.cpp:802-885) and filter_2pole_multinotch (:887-986), use_saturator == false, restated in
NumPy: the per-frame rows, the reference's fp32 loop with its double promotions, the same loop in fp64 from the SAME fp32 rows (the "truth"),
and the fp64 state-space form ( A_t, b_t, c_t, d_t ) the device scans (flan_amd/csrc/multinotch.hip).  No GPU, no flan_amd.
Also the case table the CPU and the GPU tests share; every expected result is computed once per process and handed out read-only."""
import functools
import math

import numpy as np

F32, F64 = np.float32, np.float64
ONE_POLE, TWO_POLE = 0, 1
MAX_D = 16
# device against the fp32 restatement, divided by the rms and the peak of the INPUT, per kind of input: twice the worst measured on the MI355X
# over the case table and the forced runs
REL_RMS_BOUND = {"noise": 1.83e-5, "impulse": 5.6e-6, "step": 1.06e-6}       # measured 9.133e-6, 2.754e-6, 5.257e-7
REL_MAX_BOUND = {"noise": 1.66e-5, "impulse": 7.5e-7, "step": 3.3e-6}       # measured 8.316e-6, 3.725e-7, 1.609e-6
# device against the fp64 truth: at most 4 x the restatement's own distance on the same case, or 8 fp32 ulps of the output's peak
TRUTH_FACTOR = 4.0
TRUTH_FLOOR_ULPS = 8 * 2.0 ** -23


def rows(n, sr, cutoff, damping, feedback, wet_dry, invert):
    """the per-frame fp32 rows shared by all channels: g (:814, :829, :833: the clamp by two comparisons, tan the fp64 function of the fp32
    product rounded once), R, inv * k, mix"""
    T_half = F32(math.acos(-1.0)) / F32(sr)
    nyquist = F32(sr) / F32(2)
    c = np.broadcast_to(np.asarray(cutoff, F32), (n,))
    c = np.where(c < F32(1), F32(1), np.where(nyquist < c, nyquist, c)).astype(F32)
    with np.errstate(all="ignore"):
        w = np.tan((T_half * c).astype(F64)).astype(F32) / T_half
        g = (w * T_half).astype(F32)
    R = np.broadcast_to(np.asarray(damping, F32), (n,)).astype(F32)
    ik = (F32(-1 if invert else 1) * np.broadcast_to(np.asarray(feedback, F32), (n,))).astype(F32)
    mix = np.broadcast_to(np.asarray(wet_dry, F32), (n,)).astype(F32)
    assert g.dtype == F32 and ik.dtype == F32
    return g, R, ik, mix


def _loop(x, kind, order, g_row, R_row, ik_row, mix_row, invert, dtype):
    """the reference's loop over the frames, every channel at once.  dtype F32: one fp32 rounding per operation, pow( G, i ) the DOUBLE
    function, the memory sum a double product and a double sum rounded to float at every term, the denominator a double and the quotient
    rounded once.  dtype F64: everything in fp64 from the same fp32 rows.  -> ( y, x_bar )"""
    ch, n = x.shape
    T = dtype
    exact32 = dtype is F32
    inv = T(-1 if invert else 1)
    one, two, four = T(1), T(2), T(4)
    s1 = [np.zeros(ch, T) for _ in range(order)]
    s2 = [np.zeros(ch, T) for _ in range(order)]
    y_out, xb_out = np.zeros((ch, n), T), np.zeros((ch, n), T)
    xs = x.astype(T)
    with np.errstate(all="ignore"):
        for f in range(n):
            g, R, ik, mix = T(g_row[f]), T(R_row[f]), T(ik_row[f]), T(mix_row[f])
            xf = xs[:, f]
            if kind == ONE_POLE:
                G = (g - one) / (g + one)
            else:
                d = one / (one + two * R * g + g * g)
                G = d * (one - two * R * g + g * g)
            Gd = float(G)
            ms = np.zeros(ch, T)
            for i in range(order):
                j = order - 1 - i
                term = s1[j] if kind == ONE_POLE else g * s2[j] - s1[j]
                pw = math.pow(Gd, i) if math.isfinite(Gd) else float("nan")
                ms = (ms.astype(F64) + F64(pw) * term.astype(F64)).astype(T)
            pwn = math.pow(Gd, order) if math.isfinite(Gd) else float("nan")
            den = F64(1.0) - F64(ik) * F64(pwn)
            if kind == ONE_POLE:
                ms = ms * (two / (one + g))
                num = xf + ik * ms
            else:
                num = xf + ik * four * R * d * ms
            xb = (num.astype(F64) / den).astype(T)
            y = xb
            if kind == ONE_POLE:
                Gs = g / (one + g)
                for j in range(order):
                    v = Gs * (y - s1[j])
                    lp = v + s1[j]
                    s1[j] = lp + v
                    y = lp - (y - lp)
            else:
                g1 = two * R + g
                for j in range(order):
                    hp = (y - g1 * s1[j] - s2[j]) * d
                    v1 = g * hp
                    bp = v1 + s1[j]
                    s1[j] = bp + v1
                    v2 = g * bp
                    lp = v2 + s2[j]
                    s2[j] = lp + v2
                    y = (lp - bp * two * R) + hp
            yb = y * inv
            out = mix * xb + (one - mix) * yb
            assert out.dtype == T and (not exact32 or ms.dtype == F32)
            y_out[:, f] = out
            xb_out[:, f] = xb
    return y_out, xb_out


def multinotch(x, sr, kind, order, cutoff, damping=1.0, feedback=0.0, wet_dry=0.5, invert=False, dtype=F32):
    """( y, x_bar ): dtype F32 the reference's loop, F64 the truth"""
    x = np.asarray(x, F32)
    assert 1 <= order and order * (kind + 1) <= MAX_D
    return _loop(x, kind, order, *rows(x.shape[1], sr, cutoff, damping, feedback, wet_dry, invert), invert, dtype)


def state_space(kind, order, g, R, ik, mix, invert):
    """one frame as s' = A s + b x, y = c . s + d x in fp64 from the fp32 values g, R, inv k, mix.  The states: s of section 0, 1, ... (1-pole),
    or s1, s2 of section 0, then of section 1, ... (2-pole).  A section is s' = F s + h u, out = G u + q . s; the cascade feeds section j with
    u_j = G^j x_bar + sum_{i < j} G^( j-1-i ) q . s_i, and x_bar = ( x + inv k W . s ) / ( 1 - inv k G^N ) with W = ( G^( N-1-i ) q )_i"""
    g, R, ik, mix = float(g), float(R), float(ik), float(mix)
    inv = -1.0 if invert else 1.0
    N = order
    if kind == ONE_POLE:
        G = (g - 1.0) / (g + 1.0)
        F, h, q = np.array([[-G]]), np.array([1.0 + G]), np.array([2.0 / (1.0 + g)])
    else:
        g1, d = 2.0 * R + g, 1.0 / (1.0 + 2.0 * R * g + g * g)
        G = d * (1.0 - 2.0 * R * g + g * g)
        F = np.array([[1.0 - 2.0 * g * d * g1, -2.0 * g * d], [2.0 * g * (1.0 - g * d * g1), 1.0 - 2.0 * g * g * d]])
        h = np.array([2.0 * g * d, 2.0 * g * g * d])
        q = 4.0 * R * d * np.array([-1.0, g])
    P = len(h)
    D = N * P
    W = np.concatenate([G ** (N - 1 - i) * q for i in range(N)])
    den = 1.0 - ik * G ** N
    A = np.zeros((D, D))
    b = np.zeros(D)
    for j in range(N):
        A[j * P:(j + 1) * P, j * P:(j + 1) * P] = F
        for i in range(j):
            A[j * P:(j + 1) * P, i * P:(i + 1) * P] = np.outer(h, G ** (j - 1 - i) * q)
        A[j * P:(j + 1) * P, :] += np.outer(h * G ** j, ik * W / den)
        b[j * P:(j + 1) * P] = h * G ** j / den
    through = mix + (1.0 - mix) * inv * G ** N
    c = through * ik * W / den + (1.0 - mix) * inv * W
    return A, b, c, through / den


def multinotch_state_space(x, sr, kind, order, cutoff, damping=1.0, feedback=0.0, wet_dry=0.5, invert=False):
    """the output by the state-space form, frame by frame in fp64"""
    x = np.asarray(x, F32).astype(F64)
    ch, n = x.shape
    g, R, ik, mix = rows(n, sr, cutoff, damping, feedback, wet_dry, invert)
    s = np.zeros((order * (kind + 1), ch))
    y = np.zeros((ch, n))
    for f in range(n):
        A, b, c, d = state_space(kind, order, g[f], R[f], ik[f], mix[f], invert)
        y[:, f] = c @ s + d * x[:, f]
        s = A @ s + np.outer(b, x[:, f])
    return y


def errors(got, want):
    """( rms, max ) of got - want, absolute"""
    d = np.asarray(got, F64) - np.asarray(want, F64)
    return float(np.sqrt(np.mean(d * d))), float(np.max(np.abs(d)))


def input_scale(x):
    """( rms, peak ) of the input"""
    x = np.asarray(x, F64)
    return float(np.sqrt(np.mean(x * x))), float(np.max(np.abs(x)))


def truth_criterion(got, want32, truth):
    """the project's truth criterion: got's distance from the truth, rms and max, is at most 4 x the fp32 restatement's own
    on the same case, or 8 fp32 ulps of the output's peak.  -> ( ok, ( t_rms, t_max, own_rms, own_max, floor ) )"""
    t_rms, t_max = errors(got, truth)
    own_rms, own_max = errors(want32, truth)
    floor = TRUTH_FLOOR_ULPS * float(np.max(np.abs(truth)))
    ok = t_rms <= max(TRUTH_FACTOR * own_rms, floor) and t_max <= max(TRUTH_FACTOR * own_max, floor)
    return ok, (t_rms, t_max, own_rms, own_max, floor)


# ---- the case table: name -> ( kind, order, frames, channels, sample rate, invert, input, parameters, run ) ------------------------------
# input: noise (normal, rms 0.3), impulse, step (DC from a quarter of the frames on).  parameters: scalars (cutoff 1000 Hz, damping 0.7,
# feedback 0.9, wet_dry 0.5) or curves (cutoff 200 -> 8000 Hz exponential, damping 0.2 -> 1.5, feedback 0.9 -> -0.9 through exactly 0 where n
# is odd, wet_dry 0 -> 1).  run: the frames per team forced (0: the library's choice); 1 puts every frame count below on several blocks.
# |feedback| <= 0.95 and damping in [0.2, 1.5] keep every case well conditioned: test_multinotch_reference.py holds the fp32 loop to 1e-4
# relative rms of the truth on each
CASES = {
    "p1_o1_n1": (ONE_POLE, 1, 1, 1, 48000.0, False, "noise", "scalars", 1),
    "p1_o2_n3": (ONE_POLE, 2, 3, 3, 44100.0, True, "noise", "curves", 1),
    "p1_o3_n255": (ONE_POLE, 3, 255, 1, 48000.0, False, "impulse", "scalars", 1),
    "p1_o8_n256": (ONE_POLE, 8, 256, 3, 48000.0, True, "noise", "curves", 1),
    "p1_o16_n257": (ONE_POLE, 16, 257, 1, 44100.0, False, "step", "scalars", 1),
    "p1_o16_n1000": (ONE_POLE, 16, 1000, 3, 48000.0, True, "noise", "curves", 1),
    "p1_o2_n1000": (ONE_POLE, 2, 1000, 1, 48000.0, False, "step", "curves", 1),
    "p1_o8_n8192": (ONE_POLE, 8, 8192, 3, 48000.0, False, "noise", "scalars", 0),
    "p1_o16_n9001": (ONE_POLE, 16, 9001, 1, 44100.0, True, "noise", "curves", 0),
    "p1_o3_n9001": (ONE_POLE, 3, 9001, 3, 48000.0, False, "impulse", "curves", 0),
    "p2_o1_n1": (TWO_POLE, 1, 1, 3, 48000.0, True, "noise", "scalars", 1),
    "p2_o1_n3": (TWO_POLE, 1, 3, 1, 44100.0, False, "step", "curves", 1),
    "p2_o3_n255": (TWO_POLE, 3, 255, 3, 48000.0, False, "noise", "curves", 1),
    "p2_o4_n256": (TWO_POLE, 4, 256, 1, 44100.0, True, "impulse", "scalars", 1),
    "p2_o8_n257": (TWO_POLE, 8, 257, 3, 48000.0, False, "noise", "scalars", 1),
    "p2_o8_n1000": (TWO_POLE, 8, 1000, 1, 48000.0, True, "noise", "curves", 1),
    "p2_o3_n1000": (TWO_POLE, 3, 1000, 3, 44100.0, True, "step", "scalars", 1),
    "p2_o4_n8192": (TWO_POLE, 4, 8192, 3, 48000.0, True, "noise", "curves", 0),
    "p2_o8_n9001": (TWO_POLE, 8, 9001, 1, 48000.0, False, "noise", "scalars", 0),
    "p2_o1_n9001": (TWO_POLE, 1, 9001, 3, 44100.0, False, "step", "curves", 0),
}
IDS = sorted(CASES)
LONG_NOISE = ("p1_o16_n9001", "p2_o4_n8192")      # the cases the forced runs are held on


def _frozen(v):
    if isinstance(v, np.ndarray):
        v.setflags(write=False)
    return v


def signal(kind, ch, n, rng):
    if kind == "noise":
        return rng.normal(0.0, 0.3, (ch, n)).astype(F32)
    x = np.zeros((ch, n), F32)
    if kind == "impulse":
        x[:, 0] = [1.0, -0.5, 0.25][:ch]
    else:
        x[:, n // 4:] = np.array([0.5, -0.25, 0.125], F32)[:ch, None]
    return x


def curves(n):
    """( cutoff, damping, feedback, wet_dry ) as rows of n floats"""
    t = np.arange(n) / max(n - 1, 1)
    return ((200.0 * (8000.0 / 200.0) ** t).astype(F32), (0.2 + 1.3 * t).astype(F32), np.linspace(0.9, -0.9, n).astype(F32),
            np.linspace(0.0, 1.0, n).astype(F32))


@functools.lru_cache(maxsize=None)
def case(name):
    kind, order, n, ch, sr, invert, sig, params, run = CASES[name]
    rng = np.random.default_rng(IDS.index(name) + 1)
    cutoff, damping, feedback, wet_dry = curves(n) if params == "curves" else (1000.0, 0.7, 0.9, 0.5)
    return {"name": name, "kind": kind, "order": order, "x": _frozen(signal(sig, ch, n, rng)), "sr": sr, "invert": invert, "input": sig, "run": run,
            "cutoff": _frozen(cutoff), "damping": _frozen(damping), "feedback": _frozen(feedback), "wet_dry": _frozen(wet_dry)}


def args(c):
    """the arguments of multinotch() after x"""
    return c["sr"], c["kind"], c["order"], c["cutoff"], c["damping"], c["feedback"], c["wet_dry"], c["invert"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """y32 / xb32 (the reference's fp32 loop) and y64 / xb64 (the truth)"""
    c = case(name)
    y32, xb32 = multinotch(c["x"], *args(c), dtype=F32)
    y64, xb64 = multinotch(c["x"], *args(c), dtype=F64)
    return {key: _frozen(v) for key, v in {"y32": y32, "xb32": xb32, "y64": y64, "xb64": xb64}.items()}


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == F32 and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
