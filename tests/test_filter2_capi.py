"""The C ABI of Audio::filter_2pole_* and the shelves (include/flanhip.h, flan_amd/csrc/filter.hip) without a device: symbols, constants,
workspace sizes, refusals."""
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
SYMBOLS = ["flanhip_filter2_workspace_bytes", "flanhip_filter2", "flanhip_filter2_dev"]
KINDS = ("1POLE_LOWSHELF", "1POLE_HIGHSHELF", "LOW", "BAND", "HIGH", "NOTCH", "LOWSHELF", "BANDSHELF", "HIGHSHELF")


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
    for name in ("filter2", "filter2_dev", "filter2_workspace_bytes"):
        assert callable(getattr(fa, name))
    for value, name in enumerate(KINDS):
        assert getattr(fa, "FILTER2_" + name) == value
        assert "#define FLANHIP_FILTER2_%s" % name in header
        assert int(header.split("#define FLANHIP_FILTER2_%s" % name)[1].split()[0]) == value


def test_workspace_bytes_follow_the_layout():
    def want(ch, n, run):
        blocks = -(-n // (256 * run))
        return 12 * (-(-n // 4) * 4) + 64 * ch * blocks                # the rows g, R and m, then a map (48) and a state (16) per channel and block
    for n in (1, 4095, 4096, 4097, 12305, 2880000):
        for ch in (1, 3):
            assert fa.filter2_workspace_bytes(ch, n) == want(ch, n, 16), (ch, n)
    with fa.filter_run_forced(3):
        assert fa.filter2_workspace_bytes(3, 12305) == want(3, 12305, 3)
    with fa.filter_run_forced(1000):                                   # taken as 64
        assert fa.filter2_workspace_bytes(2, 100000) == want(2, 100000, 64)
    assert fa.filter2_workspace_bytes(3, 12305) == want(3, 12305, 16)               # the hook went back
    for ch, n in ((0, 1000), (-1, 1000), (2, 0), (2, -5), (2, (1 << 36) + 1), ((1 << 20) + 1, 1000)):
        assert fa.filter2_workspace_bytes(ch, n) == 0, (ch, n)


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    out = np.zeros((2, 100), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    bad = fa.ERR_INVALID_ARG
    low = fa.FILTER2_LOW
    curves = (None, 1000.0, None, 0.5, None, 6.0)

    def refused(rc, words):
        assert rc == bad
        assert words in fa.last_error(), fa.last_error()
    refused(L.flanhip_filter2(None, 2, 100, 48000.0, *curves, low, 1, p(out), None), "null buffer")
    refused(L.flanhip_filter2(p(x), 2, 100, 48000.0, *curves, low, 1, None, None), "null buffer")
    refused(L.flanhip_filter2(p(x), 0, 100, 48000.0, *curves, low, 1, p(out), None), "non-positive size")
    refused(L.flanhip_filter2(p(x), -2, 100, 48000.0, *curves, low, 1, p(out), None), "non-positive size")
    refused(L.flanhip_filter2(p(x), 2, 0, 48000.0, *curves, low, 1, p(out), None), "non-positive size")
    refused(L.flanhip_filter2(p(x), 2, -3, 48000.0, *curves, low, 1, p(out), None), "non-positive size")
    refused(L.flanhip_filter2(p(x), 2, 100, 0.0, *curves, low, 1, p(out), None), "sample rate")
    refused(L.flanhip_filter2(p(x), 2, 100, -48000.0, *curves, low, 1, p(out), None), "sample rate")
    refused(L.flanhip_filter2(p(x), 2, 100, 48000.0, *curves, 9, 1, p(out), None), "kind")
    refused(L.flanhip_filter2(p(x), 2, 100, 48000.0, *curves, -1, 1, p(out), None), "kind")
    refused(L.flanhip_filter2(p(x), 2, 100, 48000.0, *curves, low, -1, p(out), None), "order")
    refused(L.flanhip_filter2(p(x), 2, 100, 48000.0, *curves, fa.FILTER2_HIGHSHELF, 65536, p(out), None), "order")
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    other = ctypes.c_void_p((1 << 40) + 4096)
    refused(L.flanhip_filter2_dev(None, 2, 100, 48000.0, *curves, low, 1, other, ws, None), "null buffer")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, low, 1, None, ws, None), "null buffer")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, low, 1, other, None, None), "null workspace")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, low, 0, other, None, None), "null workspace")
    refused(L.flanhip_filter2_dev(ws, 0, 100, 48000.0, *curves, low, 1, other, ws, None), "non-positive size")
    refused(L.flanhip_filter2_dev(ws, 2, 0, 48000.0, *curves, low, 1, other, ws, None), "non-positive size")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 0.0, *curves, low, 1, other, ws, None), "sample rate")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, 12, 1, other, ws, None), "kind")
    refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, fa.FILTER2_1POLE_LOWSHELF, 65536, other, ws, None), "order")
    # the notch reads the input after the cascade has run in place: out may not be the input, at any order
    for order in (0, 1, 4):
        refused(L.flanhip_filter2_dev(ws, 2, 100, 48000.0, *curves, fa.FILTER2_NOTCH, order, ws, other, None), "aliases")


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros((2, 100), np.float32)
    for kind, order in ((fa.FILTER2_LOW, 3), (fa.FILTER2_HIGH, 0), (fa.FILTER2_NOTCH, 0), (fa.FILTER2_1POLE_HIGHSHELF, 0), (fa.FILTER2_BANDSHELF, 65535)):
        with pytest.raises(fa.FlanHipError) as e:
            fa.filter2(x, 48000.0, 1000.0, 0.5, 6.0, kind=kind, order=order)
        assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.filter2(x, 48000.0, np.full(100, 1000.0, np.float32), np.full(100, 0.5, np.float32), np.full(100, 6.0, np.float32), kind=fa.FILTER2_LOWSHELF, order=2)
    assert e.value.code == fa.ERR_NO_DEVICE
    ws = ctypes.c_void_p(1 << 40)
    other = ctypes.c_void_p((1 << 40) + 4096)
    assert fa.lib.flanhip_filter2_dev(ws, 2, 100, 48000.0, None, 1000.0, None, 0.5, None, 6.0, fa.FILTER2_LOW, 1, other, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_filter2_dev(ws, 2, 100, 48000.0, ws, 0.0, ws, 0.0, ws, 0.0, fa.FILTER2_HIGHSHELF, 0, ws, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_filter2_dev(ws, 2, 100, 48000.0, None, 1000.0, None, 0.5, None, 6.0, fa.FILTER2_NOTCH, 2, other, ws, None) == fa.ERR_NO_DEVICE
