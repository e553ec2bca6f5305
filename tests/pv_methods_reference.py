"""The case table of tests/cpp/pv_methods_test.cpp (TEST INFRASTRUCTURE ONLY).

The driver calls the C++ flan::PV methods with callables written in + - * /, comparisons and selects on floats only; this module restates
every callable in NumPy float32 (bit for bit the same arithmetic), every length rule of flan_amd/host/PV.cpp from the reference line it
cites, and computes each case's expected result with tests/oracle_lib.py.  A case is a name, the PV method it holds, the input it runs
on, how it is compared and a function from the inputs to { file suffix: ( format, array or None ) } -- None is a null PV.

Left out: a non-affine shaper for PV::shape.  The oracle offers the placement rule only together with the affine shaper
(oracle_shape_affine); holding another shaper would mean restating the placement algorithm here.
"""
import struct

import numpy as np

import oracle_lib as O

f32 = np.float32

# every method of include/flan/PV.h from modify to join (tests/test_pv_methods_reference.py holds this list to the header)
METHODS = ["modify", "modify_frequency", "modify_time", "repitch", "stretch", "shape", "shape_affine", "replace_amplitudes",
           "subtract_amplitudes", "retain_n_loudest_partials", "remove_n_loudest_partials", "resonate", "desample", "time_extrapolate",
           "get_frame", "select", "freeze", "stretch_spline", "smear_time", "add_octaves", "add_harmonics", "cut_frames",
           "split_at_times", "join"]

INTERP = {"linear": 0, "midpoint": 1, "nearest": 2, "floor": 3, "ceil": 4, "smoothstep": 5, "smootherstep": 6, "sqrt": 7, "sine": 8}


# ----------------------------------------------------------------------------------------------------------------------
# formats, files, inputs
# ----------------------------------------------------------------------------------------------------------------------
class Fmt:
    def __init__(self, channels, frames, bins, window, sample_rate, analysis_rate):
        self.channels, self.frames, self.bins, self.window = int(channels), int(frames), int(bins), int(window)
        self.sample_rate, self.analysis_rate = f32(sample_rate), f32(analysis_rate)

    def with_frames(self, frames):
        return Fmt(self.channels, frames, self.bins, self.window, self.sample_rate, self.analysis_rate)

    def fields(self):
        return (self.channels, self.frames, self.bins, self.window, float(self.sample_rate), float(self.analysis_rate))

    # PVBuffer.cpp:356-359, :381-384, :428-446 in float32
    @property
    def hop(self):
        return int(self.sample_rate / self.analysis_rate)

    @property
    def dft(self):
        return (self.bins - 1) * 2

    def time_to_frame(self, t):
        return f32(f32(f32(t) * self.sample_rate) / f32(self.hop))

    def frame_to_time(self, fr):
        return (np.asarray(fr, f32) / f32(self.sample_rate / f32(self.hop))).astype(f32)

    def bin_to_frequency(self, b):
        return f32(f32(f32(b) * self.sample_rate) / f32(self.dft))

    @property
    def length(self):
        return f32(self.frame_to_time(self.frames))


FORMATS = {
    "A": Fmt(2, 61, 129, 256, 48000, 750),        # hop 64: time <-> frame exact in fp32
    "X": Fmt(2, 53, 101, 200, 44100, 441),        # hop 100: 1.0f / analysis_rate is inexact
    "B": Fmt(1, 40, 65, 128, 48000, 750),         # amplitude source: fewer channels, frames and bins
    "BIG": Fmt(1, 1100, 1025, 2048, 48000, 93.75),  # 4.5 MB of grid: 4 slabs; 9 MB of MF: 2 slabs
}
assert int(f32(48000) / f32(750)) == 64 and int(f32(44100) / f32(441)) == 100 and FORMATS["BIG"].hop == 512
assert FORMATS["A"].hop == 64 and FORMATS["X"].hop == 100

_HEADER = struct.Struct("<iiiiff")
NULL_FIELDS = (0, 0, 0, 0, 0.0, 0.0)


def write_pv(path, fmt, data):
    data = np.ascontiguousarray(data, f32)
    assert data.shape == (fmt.channels, fmt.frames, fmt.bins, 2)
    with open(path, "wb") as fh:
        fh.write(_HEADER.pack(*fmt.fields()))
        fh.write(data.tobytes())


def read_pv(path):
    """( fields, array ): a PV is float32 [ch][frames][bins][2], audio (bins == 0) float32 [ch][frames]; a zero header is a null result"""
    with open(path, "rb") as fh:
        raw = fh.read()
    fields = _HEADER.unpack_from(raw)
    ch, frames, bins = fields[:3]
    body = np.frombuffer(raw, f32, offset=_HEADER.size)
    if fields == NULL_FIELDS:
        assert body.size == 0
        return fields, None
    shape = (ch, frames) if bins == 0 else (ch, frames, bins, 2)
    assert body.size == int(np.prod(shape)), (path, fields, body.size)
    return fields, body.reshape(shape)


def read_dump(path):
    """a --sample-only dump: int32 element kind (0 float32, 1 int32, 2 uint32), int32 count, the elements"""
    with open(path, "rb") as fh:
        raw = fh.read()
    kind, count = struct.unpack_from("<ii", raw)
    out = np.frombuffer(raw, (f32, np.int32, np.uint32)[kind], offset=8)
    assert out.size == count, (path, count, out.size)
    return out


def make_input(name):
    """seeded, not an analysis: magnitudes with zeros and a few negatives; frequencies the bin centre +- up to 1.5 bin widths, so a few
    are below 0 and above Nyquist"""
    fmt = FORMATS[name]
    rng = np.random.default_rng({"A": 101, "X": 202, "B": 303, "BIG": 404}[name])
    shape = (fmt.channels, fmt.frames, fmt.bins)
    m = rng.uniform(0.0, 8.0, shape)
    kind = rng.uniform(0.0, 1.0, shape)
    m[kind < 0.06] = 0.0
    m[kind > 0.985] *= -1.0
    width = float(fmt.sample_rate) / fmt.dft
    f = (np.arange(fmt.bins)[None, None, :] + rng.uniform(-1.5, 1.5, shape)) * width
    assert (f < 0).any() and (f > float(fmt.sample_rate) / 2).any() and (m == 0).any() and (m < 0).any()
    return np.stack([m, f], axis=-1).astype(f32)


_inputs = {}


def inputs():
    if not _inputs:
        for name in FORMATS:
            _inputs[name] = make_input(name)
            _inputs[name].setflags(write=False)
    return _inputs


# ----------------------------------------------------------------------------------------------------------------------
# the callables, in float32 (the C++ twins carry the same names in tests/cpp/pv_methods_test.cpp)
# ----------------------------------------------------------------------------------------------------------------------
def _c(x):
    return f32(x)


def _sel(cond, a, b):
    return np.where(cond, a, b).astype(f32)


TF_FLOAT = {   # ( t, f ) -> float
    "mt_mono": lambda t, f: t * _c(1.5) + _sel(f > _c(8000), _c(0.01), _c(0)),
    "mt_back": lambda t, f: _sel(f < _c(6000), t * _c(1.25), _c(0.06) - t * _c(0.5)),
    "mt_lastmax": lambda t, f: t * _c(0.75) + f * _c(2e-6),
    "mt_big": lambda t, f: t * _c(0.5) + f * _c(1e-5),
    "st_tf": lambda t, f: _c(1) + t * _c(4) + f * _c(2e-5),
    "st_big": lambda t, f: _c(0.5) + t * _c(0.05) + f * _c(1e-5),
    "mfq": lambda t, f: f * (_c(1) + t * _c(2)) + _c(20),
    "mfq_big": lambda t, f: f * (_c(1) + t * _c(0.02)) + _c(20),
    "rp": lambda t, f: _c(1) + t * _c(2) + f * _c(1e-5),
    "amt": lambda t, f: t * _c(20) - _c(0.3) + f * _c(2e-5),
    "dc": lambda t, f: _sel(t < _c(0.07), _c(0.6) + f * _c(4e-5), _c(1.1) - t * _c(4) - f * _c(5e-5)),
    "ds": lambda t, f: _c(1) + t * _c(30) + f * _c(1e-4),
    "sm": lambda t, f: _c(0.01) + t * _c(0.2) + f * _c(5e-7),
}
TF_INT = {     # ( t, f ) -> int: the float is truncated
    "gr": lambda t, f: np.trunc(_c(1) + t * _c(40) + f * _c(1e-4)).astype(np.int32),
}
TF_TF = {      # ( t, f ) -> ( t, f )
    "sel": lambda t, f: (_c(0.09) - t * _c(0.8) + f * _c(1e-6), f * _c(1.1) - _c(300) + t * _c(1000)),
    "md": lambda t, f: (t * _c(1.3) + _c(0.0007) + f * _c(1e-7), f * _c(1.05) + _c(37) + t * _c(100)),
    "md_long": lambda t, f: (t * _c(10000), f),
}
T_BIN = {"nl": lambda t: np.trunc(t * _c(4000) - _c(20)).astype(np.int32)}                      # Second -> Bin
T_FLOAT = {                                                                                    # Second -> float
    "sp": lambda t: _sel(t < _c(0.01), _c(-2), _sel(t < _c(0.02), _c(0.5),
                         _sel((t > _c(0.0501)) & (t < _c(0.0529)), _c(40), _c(1) + t * _c(30)))),
    "dist_rat": lambda t: _c(1) - t * t,
}
TH_FLOAT = {"hs": lambda t, h: (_c(1) - t * _c(5)) / (_c(1) + h)}                               # ( Second, Harmonic ) -> float
CONSTANTS = {"mt": 0.05, "st2": 2.0, "st_half": 0.5, "mfq": 1000.0, "rp": 1.5, "amt": 0.5, "dc": 0.5, "ds": 3.0, "sm": 0.02, "gr": 3,
             "sel": (0.03, 5000.0), "md": (0.05, 3000.0), "nl": 10, "sp": 2.5, "hs": 0.5}
SHAPER = (0.5, 0.001, 1.02, 10.0)      # mf -> { a m + b, c f + d }


def grid(fmt, name, frames=None):
    """PV::sample_function_over_domain (PV.h:31-35): argument ( x * ( 1.0f / analysis_rate ), y * bin_to_frequency( 1 ) ), [frame][bin]"""
    frames = fmt.frames if frames is None else frames
    fn = TF_FLOAT.get(name) or TF_INT.get(name)
    out = O.sample_grid(lambda t, f: np.broadcast_to(fn(t, f), (frames, fmt.bins)), frames, fmt.bins, fmt.analysis_rate, fmt.bin_to_frequency(1))
    return np.ascontiguousarray(out, np.int32 if name in TF_INT else f32)


def grid_tf(fmt, name, frames=None):
    frames = fmt.frames if frames is None else frames
    parts = [O.sample_grid(lambda t, f: np.broadcast_to(TF_TF[name](t, f)[k], (frames, fmt.bins)), frames, fmt.bins, fmt.analysis_rate,
                           fmt.bin_to_frequency(1)) for k in (0, 1)]
    return np.ascontiguousarray(np.stack(parts, axis=-1), f32)


def at_data(fmt, pv, fn):
    """a callable at every MF's own ( time, frequency ) (PVModify.cpp:263-268, :62-66): the time is frame_to_time( frame )"""
    t = fmt.frame_to_time(np.arange(fmt.frames))[None, :, None]
    return fn(t, pv[..., 1])


def per_frame_bins(fmt, name):
    """Function::sample( 0, frames, frame_to_time( 1 ) ) (PV.cpp:555)"""
    t = (np.arange(fmt.frames, dtype=f32) * fmt.frame_to_time(1)).astype(f32)
    return np.ascontiguousarray(T_BIN[name](t), np.int32)


def spline_steps(fmt, values):
    """PVModify.cpp:391-394: max( uint32( interpolation( frame * frame_to_time( 1 ) ) ), 1 ) for every frame but the last"""
    v = np.asarray(values, f32)
    u = np.where(v >= 1, np.trunc(np.where(v >= 1, v, 1)), 0).astype(np.uint32)
    return np.maximum(u, 1).astype(np.uint32)


def spline_values(fmt, name):
    t = (np.arange(fmt.frames - 1, dtype=f32) * fmt.frame_to_time(1)).astype(f32)
    return T_FLOAT[name](t)


def distribution_args(samples_2):
    """PVModify.cpp:558-560: Function::sample( -samples_2, samples_2, 1.0f / samples_2 )"""
    return (np.arange(-samples_2, samples_2).astype(f32) * f32(f32(1.0) / f32(samples_2))).astype(f32)


def harmonic_count(fmt, mode):
    """PV.cpp:412: ceil( log2( get_height() ) ) octaves; :418: num_bins harmonics"""
    return int(np.ceil(np.log2(fmt.bin_to_frequency(fmt.bins)))) if mode == 0 else fmt.bins


def harmonic_series(fmt, name, H):
    """PV.cpp:371-379: series( { frame_to_time( frame ), harmonic } ), [frame][harmonic]"""
    t = fmt.frame_to_time(np.arange(fmt.frames))[:, None]
    h = np.arange(H, dtype=f32)[None, :]
    return np.ascontiguousarray(np.broadcast_to(TH_FLOAT[name](t, h), (fmt.frames, H)), f32)


# what --sample-only dumps, and what it must equal: { file name: array }
def sample_table():
    out = {}
    for inp in ("A", "X"):
        fmt = FORMATS[inp]
        for name in ("mt_mono", "mt_back", "mt_lastmax", "st_tf", "mfq", "rp", "amt", "ds", "sm", "gr"):
            out["grid.%s.%s" % (name, inp)] = grid(fmt, name)
        for name in ("md", "md_long"):
            out["grid.%s.%s" % (name, inp)] = grid_tf(fmt, name)
        out["outgrid.dc.%s" % inp] = grid(fmt, "dc", 2 * fmt.frames)          # resonate and select sample over the OUTPUT's frames
        out["outgrid.sel.%s" % inp] = grid_tf(fmt, "sel", 2 * fmt.frames)
        out["bins.nl.%s" % inp] = per_frame_bins(fmt, "nl")
        out["steps.sp.%s" % inp] = spline_steps(fmt, spline_values(fmt, "sp"))
        out["steps.const.%s" % inp] = spline_steps(fmt, np.full(fmt.frames - 1, CONSTANTS["sp"], f32))
        for mode, tag in ((0, "octaves"), (1, "harmonics")):
            out["series.hs.%s.%s" % (tag, inp)] = harmonic_series(fmt, "hs", harmonic_count(fmt, mode))
        for smear in ("const", "sm"):
            samples_2 = smear_plan(fmt, smear)[2]
            out["dist.dist_rat.%s.%s" % (smear, inp)] = T_FLOAT["dist_rat"](distribution_args(samples_2))
            out["dist.default.%s.%s" % (smear, inp)] = O.smear_distribution(samples_2)       # libm's cos on both sides: at most 1 ulp apart
    for name in ("mt_big", "st_big", "mfq_big"):
        out["grid.%s.BIG" % name] = grid(FORMATS["BIG"], name)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# expected results
# ----------------------------------------------------------------------------------------------------------------------
def smear_plan(fmt, smear):
    g = CONSTANTS["sm"] if smear == "const" else grid(fmt, smear)
    return O.smear_time_plan(fmt.frames, fmt.bins, fmt.sample_rate, fmt.hop, g)


def _fg(fmt, spec, frames=None):
    """a Function<TF, float> argument of a case: a callable's name or ( "const", value )"""
    if isinstance(spec, tuple):
        return np.full((fmt.frames if frames is None else frames, fmt.bins), spec[1], f32)
    return grid(fmt, spec, frames)


def _one(fmt, arr):
    return {"": (fmt.with_frames(arr.shape[1]), arr)} if arr is not None else {"": (None, None)}


NULL = {"": (None, None)}


def x_modify_time(inp, spec, interp="linear"):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        g = _fg(fmt, spec)
        frames = int(np.ceil(fmt.time_to_frame(g.max())))                       # PVModify.cpp:312, :315
        if frames <= 0:
            return NULL
        out = O.modify_time(pv, fmt.sample_rate, fmt.hop, g, INTERP[interp])
        assert out.shape[1] == frames
        return _one(fmt, out)
    return run


def x_stretch(inp, spec, interp="linear"):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        m = O.stretch_map(_fg(fmt, spec), fmt.sample_rate, fmt.hop)             # PVModify.cpp:376-382
        frames = int(np.ceil(fmt.time_to_frame(m.max())))                       # :312, :315
        out = O.modify_time(pv, fmt.sample_rate, fmt.hop, m, INTERP[interp])
        assert out.shape[1] == frames
        return _one(fmt, out)
    return run


def x_modify_frequency(inp, spec, interp="linear"):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        if isinstance(spec, tuple):
            in_mod = np.full(pv.shape[:3], spec[1], f32)
        else:
            in_mod = np.ascontiguousarray(np.broadcast_to(at_data(fmt, pv, TF_FLOAT[spec]), pv.shape[:3]), f32)
        return _one(fmt, O.modify_frequency(pv, fmt.sample_rate, _fg(fmt, spec), in_mod, INTERP[interp]))
    return run


def x_repitch(inp, spec, interp="linear"):
    def run(ins):
        fmt = FORMATS[inp]
        return _one(fmt, O.repitch(ins[inp], fmt.sample_rate, _fg(fmt, spec), INTERP[interp]))
    return run


def x_modify(inp, spec, interp="linear"):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        if isinstance(spec, tuple):
            g = np.ascontiguousarray(np.broadcast_to(np.array(spec[1], f32), (fmt.frames, fmt.bins, 2)))
            in_f = np.full(pv.shape[:3], spec[1][1], f32)
        else:
            g = grid_tf(fmt, spec)
            in_f = np.ascontiguousarray(np.broadcast_to(at_data(fmt, pv, TF_TF[spec])[1], pv.shape[:3]), f32)
        # PVModify.cpp:28-38: ceil of the largest time_to_frame; refused when that is more than ten minutes
        last = np.ceil((g[..., 0] * fmt.sample_rate / f32(fmt.hop)).astype(f32).max())
        if f32(last) / f32(fmt.sample_rate / f32(fmt.hop)) > f32(600):
            assert O.modify_out_frames(g, fmt.sample_rate, fmt.hop) == -2
            return NULL
        frames = max(int(last), 0)
        assert O.modify_out_frames(g, fmt.sample_rate, fmt.hop) == frames
        return _one(fmt, O.modify(pv, fmt.sample_rate, fmt.hop, g, in_f, INTERP[interp], frames))
    return run


def x_shape(inp, align):
    def run(ins):
        fmt = FORMATS[inp]
        return _one(fmt, O.shape_affine(ins[inp], fmt.sample_rate, *SHAPER, use_shift_alignment=align))
    return run


def x_amplitudes(inp, spec, subtract):
    def run(ins):
        fn = O.subtract_amplitudes if subtract else O.replace_amplitudes
        return _one(FORMATS[inp], fn(ins[inp], ins["B"], _fg(FORMATS[inp], spec)))
    return run


def x_n_loudest(inp, spec, remove):
    def run(ins):
        fmt = FORMATS[inp]
        n = spec[1] if isinstance(spec, tuple) else per_frame_bins(fmt, spec)
        return _one(fmt, O.n_loudest_partials(ins[inp], n, remove))
    return run


def resonate_frames(fmt, length):
    """PV.cpp:609-613: a negative length counts as 0; num_frames + ceil( time_to_frame( length ) )"""
    return int(f32(fmt.frames) + np.ceil(fmt.time_to_frame(max(f32(length), f32(0)))))


def x_resonate(inp, length, spec):
    def run(ins):
        fmt = FORMATS[inp]
        frames = resonate_frames(fmt, length)
        d = _fg(fmt, spec, frames)                                               # :616: over the OUTPUT's domain
        out = {}
        for mode, suffix in ((0, ""), (1, "#exact")):
            arr = O.resonate(ins[inp], fmt.sample_rate, fmt.hop, length, d, pow_mode=mode)
            assert arr.shape[1] == frames
            out[suffix] = (fmt.with_frames(frames), arr)
        return out
    return run


def x_desample(inp, spec, interp):
    def run(ins):
        return _one(FORMATS[inp], O.desample(ins[inp], _fg(FORMATS[inp], spec), INTERP[interp]))
    return run


def x_time_extrapolate(inp, start, end, ext, interp="linear"):
    def run(ins):
        fmt = FORMATS[inp]
        s = np.clip(f32(start), f32(0), fmt.length)                             # PVModify.cpp:612-617
        e = fmt.length if f32(end) == f32(-1) else f32(end)
        e = np.clip(e, f32(0), fmt.length)
        if s >= e or f32(ext) <= 0:
            return NULL
        sf, ef, xf = int(fmt.time_to_frame(s)), int(fmt.time_to_frame(e)), int(fmt.time_to_frame(ext))   # :619-621
        ef = min(ef, fmt.frames - 1)                                            # the layer's clamp (include/flan/PV.h)
        if sf >= ef or xf <= 0:
            return NULL
        frames = ef + xf                                                        # :623-624
        samples = O.time_extrapolate_interp_samples(sf, ef, frames, INTERP[interp])
        return _one(fmt, O.time_extrapolate(ins[inp], fmt.sample_rate, sf, ef, frames, samples))
    return run


def get_frame_times(fmt):
    return {"negative": f32(-0.5), "beyond": f32(10.0), "on": f32(fmt.frame_to_time(20)), "between": f32(0.0333)}


def x_get_frame(inp, which):
    def run(ins):
        fmt = FORMATS[inp]
        pos = np.clip(fmt.time_to_frame(get_frame_times(fmt)[which]), f32(0), f32(fmt.frames - 1))   # PV.cpp:28
        return _one(fmt, O.get_frame(ins[inp], float(pos)))
    return run


def x_select(inp, length, spec):
    def run(ins):
        fmt = FORMATS[inp]
        if f32(length) <= 0:
            return NULL                                                          # PV.cpp:98
        frames = int(fmt.time_to_frame(length))                                 # :100-101
        if frames <= 0:
            return NULL
        if isinstance(spec, tuple):
            sel = np.ascontiguousarray(np.broadcast_to(np.array(spec[1], f32), (frames, fmt.bins, 2)))
        else:
            sel = grid_tf(fmt, spec, frames)                                     # :103: over the OUTPUT's domain
        return _one(fmt, O.select(ins[inp], fmt.sample_rate, fmt.hop, sel))
    return run


FREEZE = {"mixed": ([0.05, 0.02, 0.02, 10.0], [0.01, 0.004, 0.008, 0.006]),     # unsorted, two on one frame, one in the last frame
          "none": ([], [])}


def x_freeze(inp, which):
    def run(ins):
        fmt = FORMATS[inp]
        times, lengths = FREEZE[which]
        return _one(fmt, O.freeze(ins[inp], fmt.sample_rate, fmt.hop, times, lengths))
    return run


def x_stretch_spline(inp, spec):
    def run(ins):
        fmt = FORMATS[inp]
        values = np.full(fmt.frames - 1, spec[1], f32) if isinstance(spec, tuple) else spline_values(fmt, spec)
        return _one(fmt, O.stretch_spline(ins[inp], spline_steps(fmt, values)))
    return run


def x_smear(inp, smear, gran, dist):
    def run(ins, dumps):
        fmt = FORMATS[inp]
        left, frames, samples_2 = smear_plan(fmt, smear)                              # PVModify.cpp:536-564
        if dist == "box":
            d = np.ones(2 * samples_2, f32)
        elif dist == "default":
            d = dumps["dist.default.%s.%s" % (smear, inp)]                      # libm's values, as the driver's own process rounds them
            assert d.shape == (2 * samples_2,)
        else:
            d = T_FLOAT[dist](distribution_args(samples_2))
        s = CONSTANTS["sm"] if smear == "const" else grid(fmt, smear)
        g = CONSTANTS["gr"] if gran == "const" else grid(fmt, gran)
        return _one(fmt, O.smear_time(ins[inp], fmt.sample_rate, fmt.hop, s, g, d, left, frames))
    run.needs_dumps = True
    return run


def x_harmonic(inp, spec, mode):
    def run(ins):
        fmt = FORMATS[inp]
        H = harmonic_count(fmt, mode)
        series = np.full((fmt.frames, H), spec[1], f32) if isinstance(spec, tuple) else harmonic_series(fmt, spec, H)
        return _one(fmt, O.harmonic_scale(ins[inp], fmt.sample_rate, series, mode))
    return run


def x_cut(inp, start, end):
    def run(ins):
        return _one(FORMATS[inp], O.cut_frames(ins[inp], start, end))
    return run


SPLIT_TIMES = [0.05, -0.01, 0.02, 0.02, 5.0, 0.001]     # unsorted, negative, repeated, past the end, inside frame 0


def x_split(inp):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        edges = [0]
        for t in sorted(f32(v) for v in SPLIT_TIMES):                            # PV.cpp:676-686
            fr = int(fmt.time_to_frame(t))
            if fr <= 0:
                continue
            if fmt.frames <= fr:
                break
            edges.append(fr)
        edges.append(fmt.frames)
        out, pieces = {}, []
        for i in range(len(edges) - 1):                                          # :690-693
            piece = O.cut_frames(pv, edges[i], edges[i + 1])
            out["#%d" % i] = (fmt.with_frames(piece.shape[1]), piece) if piece is not None else (None, None)
            if piece is not None:
                pieces.append(piece)
        out["#count"] = len(edges) - 1
        joined = O.join(pieces)
        out["#join"] = (fmt.with_frames(joined.shape[1]), joined)
        return out
    return run


def x_join(inp):
    def run(ins):
        fmt, pv = FORMATS[inp], ins[inp]
        return _one(fmt, O.join([O.cut_frames(pv, 10, 30), ins["B"], pv, O.cut_frames(pv, 0, 7)]))   # PV.cpp:698-720
    return run


class Case:
    def __init__(self, name, method, inp, expect, how="bits", source=None):
        self.name, self.method, self.inp, self.expect, self.how, self.source = name, method, inp, expect, how, source


def _cases():
    cs = []

    def add(name, method, inp, expect, how="bits", source=None):
        cs.append(Case("%s.%s" % (name, inp), method, inp, expect, how, source))

    for i in ("A", "X"):
        add("modify_time.monotone", "modify_time", i, x_modify_time(i, "mt_mono"))
        add("modify_time.backwards", "modify_time", i, x_modify_time(i, "mt_back"))
        add("modify_time.lastmax", "modify_time", i, x_modify_time(i, "mt_lastmax", "smoothstep"))
        add("modify_time.const", "modify_time", i, x_modify_time(i, ("const", CONSTANTS["mt"])))
        add("stretch.const2", "stretch", i, x_stretch(i, ("const", CONSTANTS["st2"])))
        add("stretch.const_half", "stretch", i, x_stretch(i, ("const", CONSTANTS["st_half"]), "nearest"))
        add("stretch.callable", "stretch", i, x_stretch(i, "st_tf"))
        add("stretch.callable_smootherstep", "stretch", i, x_stretch(i, "st_tf", "smootherstep"))
        add("modify_frequency.callable", "modify_frequency", i, x_modify_frequency(i, "mfq"))
        add("modify_frequency.callable_device_only", "modify_frequency", i, x_modify_frequency(i, "mfq"))
        add("modify_frequency.const", "modify_frequency", i, x_modify_frequency(i, ("const", CONSTANTS["mfq"]), "smoothstep"))
        add("repitch.callable", "repitch", i, x_repitch(i, "rp"))
        add("repitch.const", "repitch", i, x_repitch(i, ("const", CONSTANTS["rp"]), "smoothstep"))
        add("modify.callable", "modify", i, x_modify(i, "md"))
        add("modify.callable_device_only", "modify", i, x_modify(i, "md"))
        add("modify.const", "modify", i, x_modify(i, ("const", CONSTANTS["md"])))
        add("modify.ten_minutes", "modify", i, x_modify(i, "md_long"))
        for align in (False, True):
            tag = "aligned" if align else "plain"
            add("shape.%s" % tag, "shape", i, x_shape(i, align))
            add("shape.%s_device_only" % tag, "shape", i, x_shape(i, align))
            add("shape_affine.%s" % tag, "shape_affine", i, x_shape(i, align))
        for sub, method in ((False, "replace_amplitudes"), (True, "subtract_amplitudes")):
            add("%s.callable" % method, method, i, x_amplitudes(i, "amt", sub))
            add("%s.const" % method, method, i, x_amplitudes(i, ("const", CONSTANTS["amt"]), sub))
        for rem, method in ((False, "retain_n_loudest_partials"), (True, "remove_n_loudest_partials")):
            add("%s.callable" % method, method, i, x_n_loudest(i, "nl", rem))
            add("%s.const" % method, method, i, x_n_loudest(i, ("const", CONSTANTS["nl"]), rem))
        add("resonate.zero_const", "resonate", i, x_resonate(i, 0.0, ("const", CONSTANTS["dc"])), "resonate_const")
        add("resonate.negative_const", "resonate", i, x_resonate(i, -0.3, ("const", CONSTANTS["dc"])), "resonate_const")
        add("resonate.fractional_const", "resonate", i, x_resonate(i, 0.0301, ("const", CONSTANTS["dc"])), "resonate_const")
        add("resonate.fractional_callable", "resonate", i, x_resonate(i, 0.0301, "dc"), "resonate_grid")
        add("resonate.zero_callable", "resonate", i, x_resonate(i, 0.0, "dc"), "resonate_grid")
        add("desample.callable_linear", "desample", i, x_desample(i, "ds", "linear"))
        add("desample.callable_smoothstep", "desample", i, x_desample(i, "ds", "smoothstep"))
        add("desample.const", "desample", i, x_desample(i, ("const", CONSTANTS["ds"]), "linear"))
        add("time_extrapolate.default_end", "time_extrapolate", i, x_time_extrapolate(i, 0.02, -1, 0.03))
        add("time_extrapolate.outside", "time_extrapolate", i, x_time_extrapolate(i, -1.0, 5.0, 0.0171))
        add("time_extrapolate.inner", "time_extrapolate", i, x_time_extrapolate(i, 0.0131, 0.0577, 0.05, "smoothstep"))
        add("time_extrapolate.refuse_order", "time_extrapolate", i, x_time_extrapolate(i, 0.05, 0.01, 0.03))
        add("time_extrapolate.refuse_length", "time_extrapolate", i, x_time_extrapolate(i, 0.01, 0.05, 0.0))
        for which in ("negative", "beyond", "on", "between"):
            add("get_frame.%s" % which, "get_frame", i, x_get_frame(i, which))
        add("select.shorter", "select", i, x_select(i, 0.04, "sel"))
        add("select.longer", "select", i, x_select(i, 0.15, "sel"))
        add("select.const", "select", i, x_select(i, 0.0507, ("const", CONSTANTS["sel"])))
        add("select.refuse", "select", i, x_select(i, 0.0, "sel"))
        add("freeze.mixed", "freeze", i, x_freeze(i, "mixed"))
        add("freeze.none", "freeze", i, x_freeze(i, "none"))
        add("stretch_spline.callable", "stretch_spline", i, x_stretch_spline(i, "sp"))
        add("stretch_spline.const", "stretch_spline", i, x_stretch_spline(i, ("const", CONSTANTS["sp"])))
        add("smear_time.const_const_default", "smear_time", i, x_smear(i, "const", "const", "default"))
        add("smear_time.callable_callable_rational", "smear_time", i, x_smear(i, "sm", "gr", "dist_rat"))
        add("smear_time.const_callable_box", "smear_time", i, x_smear(i, "const", "gr", "box"))
        add("smear_time.callable_const_default", "smear_time", i, x_smear(i, "sm", "const", "default"))
        for mode, method in ((0, "add_octaves"), (1, "add_harmonics")):
            add("%s.callable" % method, method, i, x_harmonic(i, "hs", mode))
            add("%s.const" % method, method, i, x_harmonic(i, ("const", CONSTANTS["hs"]), mode))
        add("cut_frames.inner", "cut_frames", i, x_cut(i, 10, 30))
        add("cut_frames.clamped", "cut_frames", i, x_cut(i, -5, 1000))
        add("cut_frames.empty", "cut_frames", i, x_cut(i, 30, 30))
        add("cut_frames.reversed", "cut_frames", i, x_cut(i, 40, 20))
        add("split_at_times.mixed", "split_at_times", i, x_split(i))
        add("join.mixed", "join", i, x_join(i))
        for src in ("input", "stretch.const2", "stretch.callable", "shape.plain", "shape_affine.plain"):
            add("convert_to_audio.%s" % src, "convert_to_audio", i, None, "audio_rms", "%s.%s" % (src, i) if src != "input" else None)
    add("stretch.callable_big", "stretch", "BIG", x_stretch("BIG", "st_big"))
    add("modify_time.callable_big", "modify_time", "BIG", x_modify_time("BIG", "mt_big"))
    add("shape.plain", "shape", "BIG", x_shape("BIG", False))
    add("shape.plain_device_only", "shape", "BIG", x_shape("BIG", False))
    add("modify_frequency.callable_big", "modify_frequency", "BIG", x_modify_frequency("BIG", "mfq_big"))
    add("modify_frequency.callable_big_device_only", "modify_frequency", "BIG", x_modify_frequency("BIG", "mfq_big"))
    return cs


CASES = _cases()
