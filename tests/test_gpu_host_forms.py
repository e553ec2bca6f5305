"""The host form of every C-ABI family (host pointers and a cancel flag) against its `_dev` form (device pointers and a stream): a call that
finds the cancel word raised returns FLANHIP_ERR_CANCELLED and leaves its output alone, and a call that runs writes bit for bit what the
`_dev` form writes for the same input, with a workspace of the family's `_workspace_bytes` where it has one.  The entry points are called
through fa.lib directly, so that the cancel pointer can be passed.

Shapes: 2 channels x 3000 frames at 48 kHz (3000 is no multiple of 4, 64 or 256: every vector and tail branch of the copy and apply
kernels is taken); PV forms window 512, hop 128, dft 512; SPV 64 bins."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SR = 48000.0
CH, N = 2, 3000
W, HOP, DFT = 512, 128, 512
SPV_BINS = 64
SENTINEL = 0x7FC0BEEF          # a NaN payload no kernel produces


@pytest.fixture(scope="module")
def fa():
    import flan_amd
    assert flan_amd.lib.flanhip_device_count() > 0
    return flan_amd


@pytest.fixture(scope="module")
def data(fa):
    """the inputs every case draws from, made once and never written"""
    audio = np.ascontiguousarray(O.noise(CH, N, seed=411), np.float32)
    d = {"audio": audio,
         "pv": np.ascontiguousarray(O.analyze(audio, SR, W, HOP, DFT), np.float32),               # (2, 24, 257, 2)
         "spv": fa.spv_analyze(audio, SR, SPV_BINS),                                    # (2, 3000, 64, 2)
         "ir": np.ascontiguousarray(O.noise(1, 300, seed=412), np.float32),
         "side": np.ascontiguousarray(O.noise(1, N + 1, seed=413), np.float32),
         "inv": np.array([1.0, 0.5, 2.0], np.float32)}
    for v in d.values():
        v.setflags(write=False)
    return d


def P(a):
    """void * of a numpy array, a DeviceArray or None"""
    if a is None:
        return None
    return C.c_void_p(a.ptr) if hasattr(a, "ptr") else a.ctypes.data_as(C.c_void_p)


class Form:
    """One host form and its `_dev` twin.  outs: name -> (shape, dtype) of every array the host form writes; host( outs, cancel ) calls the host
    form on numpy arrays and returns its code; dev( douts ) calls the `_dev` form on DeviceArrays of the same sizes and returns its code."""

    def __init__(self, outs, host, dev):
        self.outs, self.host, self.dev = outs, host, dev


def _analyze(fa, d):
    lib, x = fa.lib, d["audio"]
    F, bins = N // HOP + 1, DFT // 2 + 1
    frames = C.c_int64(0)
    dx = fa.DeviceArray(host=x)
    return Form({"pv": ((CH, F, bins, 2), np.float32)},
                lambda o, c: lib.flanhip_analyze(P(x), CH, N, SR, W, HOP, DFT, P(o["pv"]), C.byref(frames), c),
                lambda o: lib.flanhip_analyze_dev(P(dx), CH, N, SR, W, HOP, DFT, P(o["pv"]), None))


def _synthesize(fa, d):
    lib, pv = fa.lib, d["pv"]
    ch, F, bins, _ = pv.shape
    ar = SR / HOP
    flag = C.c_int(SENTINEL)
    dpv = fa.DeviceArray(host=pv)
    dws = fa.DeviceArray(fa.synthesize_workspace_bytes(ch, F, bins, SR, ar, W))

    def host(o, c):
        flag.value = SENTINEL
        rc = lib.flanhip_synthesize(P(pv), ch, F, bins, SR, ar, W, P(o["audio"]), C.byref(flag), c)
        o["nan"][0] = flag.value
        return rc

    def dev(o):
        fa.check(lib.flanhip_memset(P(o["nan"]), 0, 4, None))
        return lib.flanhip_synthesize_dev(P(dpv), ch, F, bins, SR, ar, W, P(o["audio"]), P(dws), P(o["nan"]), None)
    return Form({"audio": ((ch, F * HOP), np.float32), "nan": ((1,), np.int32)}, host, dev)


def _modify_time(fa, d):
    lib, pv = fa.lib, d["pv"]
    ch, F, bins, _ = pv.shape
    # the identity map: every frame's own time, frame / ( sample rate / hop ) in fp32
    mod = np.ascontiguousarray(np.repeat((np.arange(F, dtype=np.float32) / np.float32(SR / HOP))[:, None], bins, axis=1))
    Fo = lib.flanhip_modify_time_out_frames(P(mod), F, bins, SR, HOP)
    assert Fo > 0
    dpv, dmod = fa.DeviceArray(host=pv), fa.DeviceArray(host=mod)
    return Form({"pv": ((ch, Fo, bins, 2), np.float32)},
                lambda o, c: lib.flanhip_modify_time(P(pv), ch, F, bins, SR, HOP, P(mod), Fo, P(o["pv"]), c),
                lambda o: lib.flanhip_modify_time_dev(P(dpv), ch, F, bins, SR, HOP, P(dmod), Fo, P(o["pv"]), None))


def _modify_frequency(fa, d):
    lib, pv = fa.lib, d["pv"]
    ch, F, bins, _ = pv.shape
    # the identity map: every bin's own frequency, and every MF's own frequency where the map is sampled at the MF
    mod = np.ascontiguousarray(np.repeat((np.arange(bins, dtype=np.float32) * np.float32(SR) / np.float32(DFT))[None, :], F, axis=0))
    inm = np.ascontiguousarray(pv[..., 1])
    dpv, dmod, dinm = fa.DeviceArray(host=pv), fa.DeviceArray(host=mod), fa.DeviceArray(host=inm)
    return Form({"pv": (pv.shape, np.float32)},
                lambda o, c: lib.flanhip_modify_frequency(P(pv), ch, F, bins, SR, P(mod), P(inm), P(o["pv"]), c),
                lambda o: lib.flanhip_modify_frequency_dev(P(dpv), ch, F, bins, SR, P(dmod), P(dinm), P(o["pv"]), None))


def _shape_affine(fa, d, align):
    lib, pv = fa.lib, d["pv"]
    ch, F, bins, _ = pv.shape
    a, b, c_, d_ = 1.0, 0.1, 0.5, -50.0                  # test_gpu_processors.py::test_shape_affine's third shaper
    dpv = fa.DeviceArray(host=pv)
    return Form({"pv": (pv.shape, np.float32)},
                lambda o, c: lib.flanhip_shape_affine(P(pv), ch, F, bins, SR, a, b, c_, d_, align, P(o["pv"]), c),
                lambda o: lib.flanhip_shape_affine_dev(P(dpv), ch, F, bins, SR, a, b, c_, d_, align, P(o["pv"]), None))


def _resample(fa, d):
    lib, x = fa.lib, d["audio"]
    dst = 44100.0
    n_out = lib.flanhip_resample_out_frames(N, SR, dst)
    dx = fa.DeviceArray(host=x)
    return Form({"audio": ((CH, n_out), np.float32)},
                lambda o, c: lib.flanhip_resample(P(x), CH, N, SR, dst, P(o["audio"]), c),
                lambda o: lib.flanhip_resample_dev(P(dx), CH, N, SR, dst, P(o["audio"]), None))


def _spv_analyze(fa, d):
    lib, x = fa.lib, d["audio"]
    dx = fa.DeviceArray(host=x)
    return Form({"spv": ((CH, N, SPV_BINS, 2), np.float32)},
                lambda o, c: lib.flanhip_spv_analyze(P(x), CH, N, SR, SPV_BINS, P(o["spv"]), c),
                lambda o: lib.flanhip_spv_analyze_dev(P(dx), CH, N, SR, SPV_BINS, P(o["spv"]), None))


def _spv_synthesize(fa, d):
    lib, spv = fa.lib, d["spv"]
    dspv = fa.DeviceArray(host=spv)
    dws = fa.DeviceArray(fa.spv_synthesize_workspace_bytes(CH, N, SPV_BINS, SR))
    return Form({"audio": ((CH, N), np.float32)},
                lambda o, c: lib.flanhip_spv_synthesize(P(spv), CH, N, SPV_BINS, SR, P(o["audio"]), c),
                lambda o: lib.flanhip_spv_synthesize_dev(P(dspv), CH, N, SPV_BINS, SR, P(o["audio"]), P(dws), None))


def _convolve(fa, d, normalize):
    lib, x, ir = fa.lib, d["audio"], d["ir"]
    irch, m = ir.shape
    dx, dir_ = fa.DeviceArray(host=x), fa.DeviceArray(host=ir)
    dws = fa.DeviceArray(fa.convolve_workspace_bytes(CH, N, irch, m))
    return Form({"audio": ((CH, fa.convolve_out_frames(N, m)), np.float32)},
                lambda o, c: lib.flanhip_convolve(P(x), CH, N, P(ir), irch, m, SR, normalize, P(o["audio"]), c),
                lambda o: lib.flanhip_convolve_dev(P(dx), CH, N, P(dir_), irch, m, SR, normalize, P(o["audio"]), P(dws), None))


def _audio_repitch(fa, d):
    lib, x, inv = fa.lib, d["audio"], d["inv"]
    g, q = 1000, fa.REPITCH_SINC
    n_out = fa.audio_repitch_out_frames(inv, g)
    dx = fa.DeviceArray(host=x)
    dws = fa.DeviceArray(fa.audio_repitch_workspace_bytes(N, SR, inv, g, q))
    return Form({"audio": ((CH, n_out), np.float32)},
                lambda o, c: lib.flanhip_audio_repitch(P(x), CH, N, SR, P(inv), inv.size, g, q, P(o["audio"]), c),
                lambda o: lib.flanhip_audio_repitch_dev(P(dx), CH, N, SR, P(inv), inv.size, g, q, P(o["audio"]), P(dws), None))


def _compress(fa, d, own_side, want_gain):
    lib, x = fa.lib, d["audio"]
    side = x if own_side else d["side"]
    sch, sn = side.shape
    params = [None, -20.0, None, 3.0, None, 0.005, None, 0.1, None, 0.0]           # threshold dB, ratio, attack s, release s, knee: all scalars
    dx = fa.DeviceArray(host=x)
    dside = dx if own_side else fa.DeviceArray(host=side)
    dws = fa.DeviceArray(fa.compress_workspace_bytes(N))
    outs = {"audio": ((CH, N), np.float32)}
    if want_gain:
        outs["gain"] = ((N,), np.float32)
    return Form(outs,
                lambda o, c: lib.flanhip_compress(P(x), CH, N, SR, P(side), sch, sn, *params, P(o["audio"]), P(o.get("gain")), c),
                lambda o: lib.flanhip_compress_dev(P(dx), CH, N, SR, P(dside), sch, sn, *params, P(o["audio"]), P(o.get("gain")), P(dws), None))


FORMS = {
    "analyze": _analyze,
    "synthesize": _synthesize,
    "modify_time": _modify_time,
    "modify_frequency": _modify_frequency,
    "shape_affine": lambda fa, d: _shape_affine(fa, d, 0),
    "shape_affine-aligned": lambda fa, d: _shape_affine(fa, d, 1),
    "resample": _resample,
    "spv_analyze": _spv_analyze,
    "spv_synthesize": _spv_synthesize,
    "convolve": lambda fa, d: _convolve(fa, d, 0),
    "convolve-normalized": lambda fa, d: _convolve(fa, d, 1),
    "audio_repitch": _audio_repitch,
    "compress-own-sidechain": lambda fa, d: _compress(fa, d, True, False),
    "compress-sidechain": lambda fa, d: _compress(fa, d, False, False),
    "compress-gain-out": lambda fa, d: _compress(fa, d, True, True),
}


def sentinel_outputs(form):
    return {k: np.full(shape, SENTINEL, np.uint32).view(np.int32) for k, (shape, dtype) in form.outs.items()}


@pytest.mark.parametrize("name", sorted(FORMS))
def test_cancelled_before_the_call(fa, data, name):
    form = FORMS[name](fa, data)
    outs = sentinel_outputs(form)
    cancel = C.c_int(1)
    rc = form.host(outs, C.cast(C.byref(cancel), C.c_void_p))
    assert rc == fa.ERR_CANCELLED, (rc, fa.last_error())
    for k, a in outs.items():                             # (synthesize: the caller's NaN flag word is an output too)
        assert np.all(a.view(np.uint32) == SENTINEL), k


@pytest.mark.parametrize("name", sorted(FORMS))
def test_host_form_equals_device_form(fa, data, name):
    form = FORMS[name](fa, data)
    outs = sentinel_outputs(form)
    cancel = C.c_int(0)
    fa.check(form.host(outs, C.cast(C.byref(cancel), C.c_void_p)))
    douts = {k: fa.DeviceArray(host=sentinel_outputs(form)[k]) for k in form.outs}
    fa.check(form.dev(douts))
    for k, (shape, dtype) in form.outs.items():
        got = outs[k]
        ref = douts[k].to_host(shape, np.int32)
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), "%s: %d of %d words differ" % (k, int(np.sum(got != ref)), got.size)
        if k != "nan":
            assert not np.all(got.view(np.uint32) == SENTINEL), k        # it was written
    if name == "synthesize":
        assert outs["nan"][0] == 0
