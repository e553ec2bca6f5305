"""The C ABI of Audio::get_local_wavelengths and its family (include/flanhip.h, flan_amd/csrc/pitch.hip) without a device: symbols, the
host-only functions bit for bit against the restatement (tests/pitch_reference.py), refusals, FLANHIP_ERR_NO_DEVICE."""
import ctypes
import os

import numpy as np
import pytest

import pitch_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_audio_local_wavelengths_count", "flanhip_audio_local_wavelengths_workspace_bytes", "flanhip_audio_yin_dprime_dev",
           "flanhip_audio_yin_pick_dev", "flanhip_audio_local_wavelengths_dev", "flanhip_audio_local_wavelength_dev",
           "flanhip_audio_local_wavelengths", "flanhip_wavelength_continuity", "flanhip_average_wavelength"]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
        assert name + "(" in header, name
    for name in ("local_wavelengths", "local_wavelengths_dev", "local_wavelength_dev", "local_wavelengths_count", "local_wavelengths_workspace_bytes",
                 "yin_dprime_dev", "yin_pick_dev", "wavelength_continuity", "average_wavelength"):
        assert callable(getattr(fa, name))
    for cited in ("AudioInformation.cpp:18-75", "DSPUtility.cpp:37-147", ":168-229", ":190-226", ":245-265"):
        assert cited in header, cited
    assert "pitch.hip" in open(os.path.join(ROOT, "flan_amd", "build.py")).read()


def test_count_is_the_restatement_s():
    for frames in (0, 1, 5, 6, 7, 40, 2048, 2049, 2176, 2177, 16000, 2880000):
        for window, hop in ((2048, 128), (256, 32), (101, 25), (6, 1), (1, 1), (16384, 7), (20000, 128)):
            for start, end in ((0, -1), (0, frames), (3, -1), (frames // 3, frames - frames // 4), (frames, -1), (frames + 5, -1)):
                if frames > 100000 and hop < 25:
                    continue
                assert fa.local_wavelengths_count(frames, start, end, window, hop) == R.count(frames, start, end, window, hop), (frames, window, hop, start, end)
    assert fa.local_wavelengths_count(16000) == 109
    assert fa.local_wavelengths_count(10, 9, -1, (1 << 63) - 1, 1) == 0 and fa.local_wavelengths_count(1 << 62, 0, -1, 1, 1 << 62) == 1      # no overflow on the way
    for bad in ((-1, 0, -1, 2048, 128), (100, -1, -1, 6, 1), (100, 0, 101, 6, 1), (100, 0, -2, 6, 1), (100, 0, -1, 0, 1), (100, 0, -1, 6, 0), (100, 0, -1, 6, -3)):
        assert fa.local_wavelengths_count(*bad) == -1, bad
        assert fa.local_wavelengths_workspace_bytes(*bad) == 0, bad
    assert fa.local_wavelengths_workspace_bytes(16000) == 16 and fa.local_wavelengths_workspace_bytes(100, 0, -1, 16384, 1) == 16
    assert fa.local_wavelengths_workspace_bytes(100000, 0, -1, 16385, 128) == 0          # a window LDS does not hold


def test_continuity_is_the_restatement_s_bit_for_bit():
    for name, v in R.CONTINUITY_VECTORS.items():
        assert R.same_bits(fa.wavelength_continuity(v, R.CONTINUITY_SR, R.CONTINUITY_HOP), R.continuity(v, R.CONTINUITY_SR, R.CONTINUITY_HOP)), name
    changed = 0
    for seed in range(200):
        v = R.random_wavelengths(seed)
        sr, hop = ((48000.0, 128), (44100.0, 256), (48000.0, 1024), (22050.0, 64))[seed % 4]
        want = R.continuity(v, sr, hop)
        assert R.same_bits(fa.wavelength_continuity(v, sr, hop), want), seed
        changed += not R.same_bits(v, want)
    assert 40 <= changed <= 190                                            # the vectors exercise the pass, and not all in one way
    assert fa.wavelength_continuity(np.zeros(0, F32), 48000.0, 128).size == 0


def test_average_is_the_restatement_s_bit_for_bit():
    cases = [([100, 0, 102, 0], 0.0, -1.0), ([100, 0, 102, -1], 0.0, -1.0), ([], 0.0, -1.0), ([0, 0, 0], 0.0, -1.0), ([-1, -1, 100], 0.5, -1.0),
             ([-1, 100, 100], 0.5, -1.0), ([100, 104], 0.0, 1.9), ([100, 104], 0.0, 2.0), ([100, 104], 1.0, -1.0), ([100, 104], 0.99, 0.0)]
    for v, ratio, sigma in cases:
        assert R.same_bits(fa.average_wavelength(np.array(v, F32), ratio, sigma), R.average(v, ratio, sigma)), (v, ratio, sigma)
    results = set()
    for seed in range(200):
        v = R.random_wavelengths(seed)
        rng = np.random.default_rng(1000 + seed)
        ratio, sigma = float(rng.choice([0.0, 0.3, 0.8, 1.0])), float(rng.choice([-1.0, 0.0, 5.0, 60.0, 1000.0]))
        want = R.average(v, ratio, sigma)
        assert R.same_bits(fa.average_wavelength(v, ratio, sigma), want), seed
        results.add("refused" if want == -1 else "mean")
    assert results == {"refused", "mean"}


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros(4000, F32)
    out = np.zeros(64, F32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    a = ctypes.c_void_p(1 << 40)                                         # never dereferenced: the refusals come first
    b = ctypes.c_void_p((1 << 40) + (1 << 30))
    w = ctypes.c_void_p((1 << 40) + (2 << 30))

    def refused(rc, words, code=None):
        assert rc == (fa.ERR_INVALID_ARG if code is None else code)
        assert words in fa.last_error(), fa.last_error()

    def host(x_, frames, start, end, window, hop, out_):
        return L.flanhip_audio_local_wavelengths(x_, frames, 48000.0, start, end, window, hop, 0.2, 10, out_, None)

    def fused(x_, frames, start, end, window, hop, out_, ws):
        return L.flanhip_audio_local_wavelengths_dev(x_, frames, start, end, window, hop, 0.2, 10, out_, ws, None)

    def dprime(x_, frames, start, end, window, hop, out_):
        return L.flanhip_audio_yin_dprime_dev(x_, frames, start, end, window, hop, out_, None)

    refused(host(None, 4000, 0, -1, 256, 32, p(out)), "null buffer")
    refused(host(p(x), 4000, 0, -1, 256, 32, None), "null buffer")
    refused(fused(None, 4000, 0, -1, 256, 32, b, w), "null buffer")
    refused(fused(a, 4000, 0, -1, 256, 32, None, w), "null buffer")
    refused(fused(a, 4000, 0, -1, 256, 32, b, None), "null workspace")
    refused(dprime(None, 4000, 0, -1, 256, 32, b), "null buffer")
    refused(dprime(a, 4000, 0, -1, 256, 32, None), "null buffer")
    for form in (lambda *s: host(p(x), *s, p(out)), lambda *s: fused(a, *s, b, w), lambda *s: dprime(a, *s, b)):
        refused(form(4000, 0, -1, 256, 0), "hop below 1")
        refused(form(4000, 0, -1, 256, -32), "hop below 1")
        refused(form(4000, -1, -1, 256, 32), "range outside the signal")
        refused(form(4000, 0, 4001, 256, 32), "range outside the signal")
        refused(form(4000, 0, -2, 256, 32), "range outside the signal")
        refused(form(4000, 0, -1, 0, 32), "non-positive size")
        refused(form(4000, 0, -1, -256, 32), "non-positive size")
        refused(form(-4000, 0, -1, 256, 32), "non-positive size")
        refused(form(40000, 0, -1, 16385, 32), "window above 16384", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_audio_yin_pick_dev(None, 4, 128, 0.2, 10, b, None), "null buffer")
    refused(L.flanhip_audio_yin_pick_dev(a, 4, 128, 0.2, 10, None, None), "null buffer")
    refused(L.flanhip_audio_yin_pick_dev(a, -4, 128, 0.2, 10, b, None), "negative size")
    refused(L.flanhip_audio_yin_pick_dev(a, 4, -128, 0.2, 10, b, None), "negative size")
    refused(L.flanhip_audio_yin_pick_dev(a, 4, 8193, 0.2, 10, b, None), "row above 8192", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_audio_local_wavelength_dev(None, 2048, 0.2, 10, b, None), "null buffer")
    refused(L.flanhip_audio_local_wavelength_dev(a, 2048, 0.2, 10, None, None), "null buffer")
    refused(L.flanhip_audio_local_wavelength_dev(a, 0, 0.2, 10, b, None), "non-positive size")
    refused(L.flanhip_audio_local_wavelength_dev(a, 16385, 0.2, 10, b, None), "window above 16384", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_wavelength_continuity(None, 5, 48000.0, 128), "null buffer")
    refused(L.flanhip_wavelength_continuity(p(out), -5, 48000.0, 128), "negative size")
    refused(L.flanhip_wavelength_continuity(p(out), 5, 48000.0, 0), "hop below 1")
    value = ctypes.c_float(0)
    refused(L.flanhip_average_wavelength(None, 5, 0.0, -1.0, ctypes.cast(ctypes.byref(value), ctypes.c_void_p)), "null buffer")
    refused(L.flanhip_average_wavelength(p(out), 5, 0.0, -1.0, None), "null buffer")
    refused(L.flanhip_average_wavelength(p(out), -5, 0.0, -1.0, ctypes.cast(ctypes.byref(value), ctypes.c_void_p)), "negative size")


def test_what_needs_no_device_asks_for_none():
    """no window at all, and windows without an interior point (h < 3): the host form answers on its own"""
    x = np.random.default_rng(6).uniform(-1, 1, 40).astype(F32)
    assert fa.local_wavelengths(x, 48000.0, 0, -1, 64, 16).size == 0       # the signal is shorter than a window
    for window in (1, 2, 3, 4, 5):
        out = fa.local_wavelengths(x, 48000.0, 0, -1, window, 1)
        assert out.size == 40 - window and np.all(out == 0)


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros(4000, F32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.local_wavelengths(x, 48000.0)
    assert e.value.code == fa.ERR_NO_DEVICE
    a, b, w = ctypes.c_void_p(1 << 40), ctypes.c_void_p((1 << 40) + (1 << 30)), ctypes.c_void_p((1 << 40) + (2 << 30))
    L = fa.lib
    assert L.flanhip_audio_local_wavelengths_dev(a, 4000, 0, -1, 256, 32, 0.2, 10, b, w, None) == fa.ERR_NO_DEVICE
    assert L.flanhip_audio_yin_dprime_dev(a, 4000, 0, -1, 256, 32, b, None) == fa.ERR_NO_DEVICE
    assert L.flanhip_audio_yin_pick_dev(a, 4, 128, 0.2, 10, b, None) == fa.ERR_NO_DEVICE
    assert L.flanhip_audio_local_wavelength_dev(a, 2048, 0.2, 10, b, None) == fa.ERR_NO_DEVICE
