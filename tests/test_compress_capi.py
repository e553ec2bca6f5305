"""The C ABI of Audio::compress / modify_volume / set_volume (include/flanhip.h, flan_amd/csrc/compress.hip) without a device: symbols,
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
SYMBOLS = ["flanhip_compress_workspace_bytes", "flanhip_compress", "flanhip_compress_dev", "flanhip_compress_debug_run",
           "flanhip_audio_gain_dev", "flanhip_audio_set_volume_workspace_bytes", "flanhip_audio_set_volume_dev"]
PARAMS = [None, -20.0, None, 3.0, None, 0.005, None, 0.1, None, 0.0]


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
    for name in ("compress", "compress_dev", "compress_workspace_bytes", "compress_run_forced", "audio_gain_dev", "audio_set_volume_dev",
                 "audio_set_volume_workspace_bytes"):
        assert callable(getattr(fa, name))


def test_workspace_bytes_follow_the_layout():
    def want(n, run):
        blocks = -(-n // (256 * run))
        return 5 * 4 * (-(-n // 4) * 4) + 56 * blocks
    for n in (1, 2, 4095, 4096, 4097, 12305, 2880000):
        assert fa.compress_workspace_bytes(n) == want(n, 16), n
    with fa.compress_run_forced(3):
        assert fa.compress_workspace_bytes(12305) == want(12305, 3)
    with fa.compress_run_forced(1000):                                # taken as 64
        assert fa.compress_workspace_bytes(100000) == want(100000, 64)
    assert fa.compress_workspace_bytes(12305) == want(12305, 16)       # the hook went back
    assert fa.compress_workspace_bytes(0) == 0
    assert fa.compress_workspace_bytes(-5) == 0
    assert fa.compress_workspace_bytes((1 << 36) + 1) == 0
    assert fa.audio_set_volume_workspace_bytes(2, 1000) == 8192
    assert fa.audio_set_volume_workspace_bytes(0, 1000) == 0
    assert fa.audio_set_volume_workspace_bytes(2, 0) == 0
    assert fa.audio_set_volume_workspace_bytes(2, -1) == 0


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    side = np.zeros((1, 100), np.float32)
    out = np.zeros((2, 100), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    bad = fa.ERR_INVALID_ARG
    assert L.flanhip_compress(None, 2, 100, 48000.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 48000.0, None, 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 48000.0, p(side), 1, 100, *PARAMS, None, None, None) == bad
    assert L.flanhip_compress(p(x), 0, 100, 48000.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 0, 48000.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, -3, 48000.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 48000.0, p(side), 0, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 48000.0, p(side), 1, 0, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 0.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, -48000.0, p(side), 1, 100, *PARAMS, p(out), None, None) == bad
    assert L.flanhip_compress(p(x), 2, 100, 48000.0, p(side), 1, 99, *PARAMS, p(out), None, None) == bad
    assert "fewer frames" in fa.last_error()
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    assert L.flanhip_compress_dev(None, 2, 100, 48000.0, ws, 1, 100, *PARAMS, ws, None, ws, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 100, 48000.0, None, 1, 100, *PARAMS, ws, None, ws, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 100, 48000.0, ws, 1, 100, *PARAMS, None, None, ws, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 100, 48000.0, ws, 1, 100, *PARAMS, ws, None, None, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 100, 48000.0, ws, 1, 99, *PARAMS, ws, None, ws, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 100, 0.0, ws, 1, 100, *PARAMS, ws, None, ws, None) == bad
    assert L.flanhip_compress_dev(ws, 2, 0, 48000.0, ws, 1, 100, *PARAMS, ws, None, ws, None) == bad
    assert L.flanhip_audio_gain_dev(None, 2, 100, None, 0.5, ws, None) == bad
    assert L.flanhip_audio_gain_dev(ws, 2, 100, None, 0.5, None, None) == bad
    assert L.flanhip_audio_gain_dev(ws, 0, 100, None, 0.5, ws, None) == bad
    assert L.flanhip_audio_gain_dev(ws, 2, 0, None, 0.5, ws, None) == bad
    assert L.flanhip_audio_set_volume_dev(None, 2, 100, 48000.0, None, 0.5, ws, ws, None) == bad
    assert L.flanhip_audio_set_volume_dev(ws, 2, 100, 48000.0, None, 0.5, None, ws, None) == bad
    assert L.flanhip_audio_set_volume_dev(ws, 2, 100, 48000.0, None, 0.5, ws, None, None) == bad
    assert L.flanhip_audio_set_volume_dev(ws, 2, 100, 0.0, None, 0.5, ws, ws, None) == bad
    assert L.flanhip_audio_set_volume_dev(ws, 2, -1, 48000.0, None, 0.5, ws, ws, None) == bad


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.zeros((2, 100), np.float32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.compress(x, 48000.0)
    assert e.value.code == fa.ERR_NO_DEVICE
    ws = ctypes.c_void_p(1 << 40)
    assert fa.lib.flanhip_compress_dev(ws, 2, 100, 48000.0, ws, 1, 100, *PARAMS, ws, None, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_audio_gain_dev(ws, 2, 100, None, 0.5, ws, None) == fa.ERR_NO_DEVICE
    assert fa.lib.flanhip_audio_set_volume_dev(ws, 2, 100, 48000.0, None, 0.5, ws, ws, None) == fa.ERR_NO_DEVICE
