"""The C ABI of the phase-difference network and the methods over it (include/flanhip.h, flan_amd/csrc/halfband.hip) without a device:
symbols, the poles, workspace sizes, refusals."""
import ctypes
import os

import numpy as np
import pytest

import halfband_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_halfband_poles", "flanhip_halfband_workspace_bytes", "flanhip_halfband_debug_run", "flanhip_hilbert", "flanhip_hilbert_dev",
           "flanhip_halfband_modulate", "flanhip_halfband_modulate_dev", "flanhip_halfband_multiply", "flanhip_halfband_multiply_dev"]


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
    for name in ("halfband_poles", "halfband_workspace_bytes", "hilbert", "hilbert_dev", "halfband_modulate", "halfband_modulate_dev",
                 "halfband_multiply", "halfband_multiply_dev", "halfband_run_forced"):
        assert callable(getattr(fa, name))


def test_the_poles_are_the_restatement_s():
    first, second = fa.halfband_poles()
    want_first, want_second = R.poles()
    for got, want in ((first, want_first), (second, want_second)):
        assert got.dtype == np.float32 and got.shape == (10,)
        d = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
        assert np.all(d <= 1), (got, want)


def test_workspace_bytes_follow_the_layout():
    def want(ch, n, run):
        blocks = -(-n // (256 * run))
        return 4 * 15 * 55 * 8 + 640 * ch * blocks                    # four cascades' tables, then their totals and states per channel and block
    assert want(1, 1, 16) == 26400 + 640
    for n in (1, 4095, 4096, 4097, 9001, 2880000):
        for ch in (1, 3):
            assert fa.halfband_workspace_bytes(ch, n) == want(ch, n, 16), (ch, n)
    with fa.halfband_run_forced(1):
        assert fa.halfband_workspace_bytes(3, 1000) == want(3, 1000, 1)
    with fa.halfband_run_forced(1000):                                 # taken as 64
        assert fa.halfband_workspace_bytes(2, 100000) == want(2, 100000, 64)
    assert fa.halfband_workspace_bytes(3, 9001) == want(3, 9001, 16)                # the hook went back
    with fa.filter_run_forced(3):                                      # the filters' hook is another
        assert fa.halfband_workspace_bytes(3, 9001) == want(3, 9001, 16)
    for ch, n in ((0, 1000), (-1, 1000), (2, 0), (2, -5), (2, (1 << 36) + 1), ((1 << 20) + 1, 1000)):
        assert fa.halfband_workspace_bytes(ch, n) == 0, (ch, n)


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    out = np.zeros((2, 100), np.float32)
    out2 = np.zeros((2, 100), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    bad = fa.ERR_INVALID_ARG
    mod = (None, 1.0, None, 0.0, None)

    def refused(rc, words):
        assert rc == bad
        assert words in fa.last_error(), fa.last_error()
    refused(L.flanhip_hilbert(None, 2, 100, 48000.0, p(out), p(out2), None), "null buffer")
    refused(L.flanhip_hilbert(p(x), 2, 100, 48000.0, None, p(out2), None), "null buffer")
    refused(L.flanhip_hilbert(p(x), 2, 100, 48000.0, p(out), None, None), "null buffer")
    refused(L.flanhip_hilbert(p(x), 0, 100, 48000.0, p(out), p(out2), None), "non-positive size")
    refused(L.flanhip_hilbert(p(x), 2, -3, 48000.0, p(out), p(out2), None), "non-positive size")
    refused(L.flanhip_hilbert(p(x), 2, 100, 0.0, p(out), p(out2), None), "sample rate")
    refused(L.flanhip_halfband_modulate(None, 2, 100, 48000.0, *mod, p(out), None), "null buffer")
    refused(L.flanhip_halfband_modulate(p(x), 2, 100, 48000.0, *mod, None, None), "null buffer")
    refused(L.flanhip_halfband_modulate(p(x), -2, 100, 48000.0, *mod, p(out), None), "non-positive size")
    refused(L.flanhip_halfband_modulate(p(x), 2, 0, 48000.0, *mod, p(out), None), "non-positive size")
    refused(L.flanhip_halfband_modulate(p(x), 2, 100, -48000.0, *mod, p(out), None), "sample rate")
    refused(L.flanhip_halfband_multiply(None, 2, 100, 48000.0, p(x), 2, 100, 44100.0, p(out), None), "null buffer")
    refused(L.flanhip_halfband_multiply(p(x), 2, 100, 48000.0, None, 2, 100, 44100.0, p(out), None), "null buffer")
    refused(L.flanhip_halfband_multiply(p(x), 2, 100, 48000.0, p(x), 2, 100, 44100.0, None, None), "null buffer")
    refused(L.flanhip_halfband_multiply(p(x), 2, 100, 48000.0, p(x), 0, 100, 44100.0, p(out), None), "non-positive size")
    refused(L.flanhip_halfband_multiply(p(x), 2, 0, 48000.0, p(x), 2, 100, 44100.0, p(out), None), "non-positive size")
    refused(L.flanhip_halfband_multiply(p(x), 2, 100, 48000.0, p(x), 2, 100, 0.0, p(out), None), "sample rate")
    assert L.flanhip_hilbert(p(x), 2, (1 << 36) + 1, 48000.0, p(out), p(out2), None) == fa.ERR_UNSUPPORTED
    assert "shape out of range" in fa.last_error()
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    other = ctypes.c_void_p((1 << 40) + 4096)
    refused(L.flanhip_hilbert_dev(None, 2, 100, 48000.0, other, other, ws, None), "null buffer")
    refused(L.flanhip_hilbert_dev(ws, 2, 100, 48000.0, None, other, ws, None), "null buffer")
    refused(L.flanhip_hilbert_dev(ws, 2, 100, 48000.0, other, None, ws, None), "null buffer")
    refused(L.flanhip_hilbert_dev(ws, 2, 100, 48000.0, other, other, None, None), "null workspace")
    refused(L.flanhip_hilbert_dev(ws, 2, 0, 48000.0, other, other, ws, None), "non-positive size")
    refused(L.flanhip_hilbert_dev(ws, 2, 100, 0.0, other, other, ws, None), "sample rate")
    refused(L.flanhip_halfband_modulate_dev(None, 2, 100, 48000.0, *mod, other, ws, None), "null buffer")
    refused(L.flanhip_halfband_modulate_dev(ws, 2, 100, 48000.0, *mod, None, ws, None), "null buffer")
    refused(L.flanhip_halfband_modulate_dev(ws, 2, 100, 48000.0, *mod, other, None, None), "null workspace")
    refused(L.flanhip_halfband_modulate_dev(ws, 2, 100, 48000.0, None, 0.0, None, 0.0, ws, other, None, None), "null workspace")
    refused(L.flanhip_halfband_modulate_dev(ws, 0, 100, 48000.0, *mod, other, ws, None), "non-positive size")
    refused(L.flanhip_halfband_modulate_dev(ws, 2, 100, 0.0, *mod, other, ws, None), "sample rate")
    refused(L.flanhip_halfband_multiply_dev(None, 2, 100, 48000.0, ws, 2, 100, 44100.0, other, ws, None), "null buffer")
    refused(L.flanhip_halfband_multiply_dev(ws, 2, 100, 48000.0, None, 2, 100, 44100.0, other, ws, None), "null buffer")
    refused(L.flanhip_halfband_multiply_dev(ws, 2, 100, 48000.0, ws, 2, 100, 44100.0, None, ws, None), "null buffer")
    refused(L.flanhip_halfband_multiply_dev(ws, 2, 100, 48000.0, ws, 2, 100, 44100.0, other, None, None), "null workspace")
    refused(L.flanhip_halfband_multiply_dev(ws, 2, 100, 48000.0, ws, 2, -1, 44100.0, other, ws, None), "non-positive size")
    refused(L.flanhip_halfband_multiply_dev(ws, 2, 100, -1.0, ws, 2, 100, 44100.0, other, ws, None), "sample rate")


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros((2, 100), np.float32)
    for call in (lambda: fa.hilbert(x, 48000.0), lambda: fa.halfband_modulate(x, 48000.0, 0.5, 0.5),
                 lambda: fa.halfband_modulate(x, 48000.0, phase=np.zeros(100, np.float32)), lambda: fa.halfband_multiply(x, 48000.0, x[:1, :50], 44100.0)):
        with pytest.raises(fa.FlanHipError) as e:
            call()
        assert e.value.code == fa.ERR_NO_DEVICE
    ws = ctypes.c_void_p(1 << 40)
    other = ctypes.c_void_p((1 << 40) + 4096)
    assert fa.lib.flanhip_hilbert_dev(ws, 2, 100, 48000.0, other, other, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_halfband_modulate_dev(ws, 2, 100, 48000.0, None, 1.0, None, 0.0, None, ws, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_halfband_multiply_dev(ws, 2, 100, 48000.0, ws, 1, 50, 44100.0, other, ws, None) == fa.ERR_NO_DEVICE
