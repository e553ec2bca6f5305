"""The C ABI of Audio::filter_1pole_multinotch / filter_2pole_multinotch (include/flanhip.h, flan_amd/csrc/multinotch.hip) without a device:
symbols, the workspace formula, refusals, FLANHIP_ERR_NO_DEVICE."""
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
SYMBOLS = ["flanhip_multinotch_workspace_bytes", "flanhip_multinotch", "flanhip_multinotch_dev", "flanhip_multinotch_debug_run"]
ONE_POLE, TWO_POLE = 0, 1


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
    for name in ("multinotch", "multinotch_dev", "multinotch_workspace_bytes", "multinotch_run_forced"):
        assert callable(getattr(fa, name))
    assert (fa.MULTINOTCH_1POLE, fa.MULTINOTCH_2POLE) == (ONE_POLE, TWO_POLE)
    assert "AudioFilter.cpp:802-885" in header and ":887-986" in header
    assert "#define FLANHIP_MULTINOTCH_1POLE 0" in header and "#define FLANHIP_MULTINOTCH_2POLE 1" in header


def want(ch, n, kind, order, run=0):
    """24 * roundup( n, 4 ) + 8 * DP * ( DP + 2 ) * ch * ceil( n / ( ( 128 / DP ) * run ) ), DP the least of 4, 8, 16 that holds the D states"""
    D = order * (kind + 1)
    DP = 4 if D <= 4 else 8 if D <= 8 else 16
    per_block = (128 // DP) * (run or 16 * DP)                          # the library's choice: 2048 frames a block
    return 24 * ((n + 3) // 4 * 4) + 8 * DP * (DP + 2) * ch * ((n + per_block - 1) // per_block)


def test_workspace_bytes_follow_the_header_s_formula():
    assert want(1, 1, ONE_POLE, 1) == 96 + 192
    assert want(8, 2880000, ONE_POLE, 16) == 24 * 2880000 + 8 * 16 * 18 * 8 * 1407
    for n in (1, 3, 255, 256, 257, 1000, 8192, 9001, 2880000, 1 << 36):
        for ch in (1, 3, 8):
            for kind, orders in ((ONE_POLE, (1, 2, 3, 4, 5, 8, 9, 16)), (TWO_POLE, (1, 2, 3, 4, 5, 8))):
                for order in orders:
                    assert fa.multinotch_workspace_bytes(ch, n, kind, order) == want(ch, n, kind, order), (ch, n, kind, order)
    for forced, run in ((1, 1), (4, 4), (16, 16), (64, 64), (1000, 64)):
        with fa.multinotch_run_forced(forced):
            for kind, order in ((ONE_POLE, 3), (ONE_POLE, 16), (TWO_POLE, 4)):
                assert fa.multinotch_workspace_bytes(3, 9001, kind, order) == want(3, 9001, kind, order, run), (forced, kind, order)
    assert fa.multinotch_workspace_bytes(3, 9001, ONE_POLE, 16) == want(3, 9001, ONE_POLE, 16)          # the hook was handed back
    for ch, n, kind, order in ((0, 1000, 0, 2), (-1, 1000, 0, 2), (2, 0, 0, 2), (2, -5, 1, 2), (2, (1 << 36) + 1, 0, 2), ((1 << 20) + 1, 1000, 0, 2),
                               (2, 1000, 2, 2), (2, 1000, -1, 2), (2, 1000, 0, 0), (2, 1000, 1, 0), (2, 1000, 0, -3), (2, 1000, 0, 17), (2, 1000, 1, 9),
                               (2, 1000, 0, 1 << 30), (2, 1000, 1, 1 << 30)):
        assert fa.multinotch_workspace_bytes(ch, n, kind, order) == 0, (ch, n, kind, order)


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    out = np.zeros((2, 100), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    par = (None, 440.0, None, 0.7, None, 0.9, None, 0.5)

    def refused(rc, words, code=None):
        assert rc == (fa.ERR_INVALID_ARG if code is None else code)
        assert words in fa.last_error(), fa.last_error()
    refused(L.flanhip_multinotch(None, 2, 100, 48000.0, *par, 0, 2, 0, p(out), None), "null buffer")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 0, 2, 0, None, None), "null buffer")
    refused(L.flanhip_multinotch(p(x), 0, 100, 48000.0, *par, 0, 2, 0, p(out), None), "non-positive size")
    refused(L.flanhip_multinotch(p(x), 2, -3, 48000.0, *par, 1, 2, 0, p(out), None), "non-positive size")
    refused(L.flanhip_multinotch(p(x), 2, 100, 0.0, *par, 0, 2, 0, p(out), None), "sample rate")
    refused(L.flanhip_multinotch(p(x), 2, 100, -48000.0, *par, 1, 2, 0, p(out), None), "sample rate")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 2, 2, 0, p(out), None), "unknown multinotch kind")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, -1, 2, 0, p(out), None), "unknown multinotch kind")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 0, 0, 0, p(out), None), "order not positive")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 1, 0, 1, p(out), None), "order not positive")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 1, -2, 1, p(out), None), "order not positive")
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 0, 17, 0, p(out), None), "more than 16 states", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 1, 9, 0, p(out), None), "more than 16 states", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch(p(x), 2, 100, 48000.0, *par, 1, 65535, 0, p(out), None), "more than 16 states", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch(p(x), (1 << 20) + 1, 100, 48000.0, *par, 0, 2, 0, p(out), None), "shape out of range", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch(p(x), 2, (1 << 36) + 1, 48000.0, *par, 0, 2, 0, p(out), None), "shape out of range", fa.ERR_UNSUPPORTED)
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    other = ctypes.c_void_p((1 << 40) + 4096)
    refused(L.flanhip_multinotch_dev(None, 2, 100, 48000.0, *par, 0, 2, 0, other, ws, None), "null buffer")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 0, 2, 0, None, ws, None), "null buffer")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 0, 2, 0, other, None, None), "null workspace")
    refused(L.flanhip_multinotch_dev(ws, 2, 0, 48000.0, *par, 0, 2, 0, other, ws, None), "non-positive size")
    refused(L.flanhip_multinotch_dev(ws, -2, 100, 48000.0, *par, 1, 2, 0, other, ws, None), "non-positive size")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 0.0, *par, 0, 2, 0, other, ws, None), "sample rate")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 5, 2, 0, other, ws, None), "unknown multinotch kind")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 0, 0, 0, other, ws, None), "order not positive")
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 0, 17, 0, other, ws, None), "more than 16 states", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch_dev(ws, 2, 100, 48000.0, *par, 1, 9, 0, other, ws, None), "more than 16 states", fa.ERR_UNSUPPORTED)
    refused(L.flanhip_multinotch_dev(ws, (1 << 20) + 1, 100, 48000.0, *par, 1, 8, 0, other, ws, None), "shape out of range", fa.ERR_UNSUPPORTED)


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros((2, 100), np.float32)
    curve = np.full(100, 440.0, np.float32)
    for call in (lambda: fa.multinotch(x, 48000.0, 440.0, order=16), lambda: fa.multinotch(x, 48000.0, curve, curve * 0 + 0.7, 0.7, curve * 0, fa.MULTINOTCH_2POLE, 8, True)):
        with pytest.raises(fa.FlanHipError) as e:
            call()
        assert e.value.code == fa.ERR_NO_DEVICE
    ws = ctypes.c_void_p(1 << 40)
    other = ctypes.c_void_p((1 << 40) + 4096)
    assert fa.lib.flanhip_multinotch_dev(ws, 2, 100, 48000.0, None, 440.0, None, 0.7, None, 0.9, None, 0.5, 1, 8, 0, other, ws, None) == fa.ERR_NO_DEVICE
