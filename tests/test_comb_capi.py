"""The C ABI of Audio::filter_comb (include/flanhip.h, flan_amd/csrc/comb.hip) without a device: symbols, the workspace formula, refusals,
FLANHIP_ERR_NO_DEVICE."""
import ctypes
import os

import numpy as np
import pytest


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_filter_comb_workspace_bytes", "flanhip_filter_comb", "flanhip_filter_comb_dev", "flanhip_filter_comb_debug_local"]


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
    for name in ("filter_comb", "filter_comb_dev", "filter_comb_workspace_bytes", "filter_comb_local_forced"):
        assert callable(getattr(fa, name))
    assert "AudioFilter.cpp:988-1043" in header


def test_workspace_bytes_follow_the_header_s_formula():
    def want(ch, n):
        return 256 + 16 * ch * n + 24 * n          # 64 words; X[2][ch][n] doubles; C[2][n] doubles and P[2][n] int32
    assert want(1, 1) == 296
    for n in (1, 2, 17, 4095, 4096, 4097, 12305, 2880000, (1 << 31) - 1):
        for ch in (1, 3, 8):
            assert fa.filter_comb_workspace_bytes(ch, n) == want(ch, n), (ch, n)
    assert fa.filter_comb_workspace_bytes(8, 2880000) == 437760256        # 8 ch x 60 s at 48 kHz
    for forced in (-1, 1, 9):                                              # the LDS level needs no workspace of its own
        with fa.filter_comb_local_forced(forced):
            assert fa.filter_comb_workspace_bytes(3, 9001) == want(3, 9001)
    for ch, n in ((0, 1000), (-1, 1000), (2, 0), (2, -5), (2, 1 << 31), (2, (1 << 36) + 1), ((1 << 20) + 1, 1000)):
        assert fa.filter_comb_workspace_bytes(ch, n) == 0, (ch, n)


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    out = np.zeros((2, 100), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    par = (None, 440.0, None, 0.7, None, 0.5, 0)

    def refused(rc, words, code=None):
        assert rc == (fa.ERR_INVALID_ARG if code is None else code)
        assert words in fa.last_error(), fa.last_error()
    refused(L.flanhip_filter_comb(None, 2, 100, 48000.0, *par, p(out), None), "null buffer")
    refused(L.flanhip_filter_comb(p(x), 2, 100, 48000.0, *par, None, None), "null buffer")
    refused(L.flanhip_filter_comb(p(x), 0, 100, 48000.0, *par, p(out), None), "non-positive size")
    refused(L.flanhip_filter_comb(p(x), 2, -3, 48000.0, *par, p(out), None), "non-positive size")
    refused(L.flanhip_filter_comb(p(x), 2, 100, 0.0, *par, p(out), None), "sample rate")
    refused(L.flanhip_filter_comb(p(x), 2, 100, -48000.0, *par, p(out), None), "sample rate")
    refused(L.flanhip_filter_comb(p(x), 2, 1 << 31, 48000.0, *par, p(out), None), "shape out of range", fa.ERR_UNSUPPORTED)   # the links are int32
    refused(L.flanhip_filter_comb(p(x), (1 << 20) + 1, 100, 48000.0, *par, p(out), None), "shape out of range", fa.ERR_UNSUPPORTED)
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    other = ctypes.c_void_p((1 << 40) + 4096)
    refused(L.flanhip_filter_comb_dev(None, 2, 100, 48000.0, *par, other, ws, None), "null buffer")
    refused(L.flanhip_filter_comb_dev(ws, 2, 100, 48000.0, *par, None, ws, None), "null buffer")
    refused(L.flanhip_filter_comb_dev(ws, 2, 100, 48000.0, *par, other, None, None), "null workspace")
    refused(L.flanhip_filter_comb_dev(ws, 2, 0, 48000.0, *par, other, ws, None), "non-positive size")
    refused(L.flanhip_filter_comb_dev(ws, -2, 100, 48000.0, *par, other, ws, None), "non-positive size")
    refused(L.flanhip_filter_comb_dev(ws, 2, 100, 0.0, *par, other, ws, None), "sample rate")
    refused(L.flanhip_filter_comb_dev(ws, 2, 1 << 31, 48000.0, *par, other, ws, None), "shape out of range", fa.ERR_UNSUPPORTED)


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros((2, 100), np.float32)
    curve = np.full(100, 440.0, np.float32)
    for call in (lambda: fa.filter_comb(x, 48000.0, 440.0), lambda: fa.filter_comb(x, 48000.0, curve, 0.7, curve * 0, True)):
        with pytest.raises(fa.FlanHipError) as e:
            call()
        assert e.value.code == fa.ERR_NO_DEVICE
    ws = ctypes.c_void_p(1 << 40)
    other = ctypes.c_void_p((1 << 40) + 4096)
    assert fa.lib.flanhip_filter_comb_dev(ws, 2, 100, 48000.0, None, 440.0, None, 0.7, None, 0.5, 0, other, ws, None) == fa.ERR_NO_DEVICE
