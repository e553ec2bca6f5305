"""Audio::convolve's C ABI (include/flanhip.h, flan_amd/csrc/conv.hip) without a device: symbols, host arithmetic, refusals."""
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
CONV_SYMBOLS = ["flanhip_convolve_out_frames", "flanhip_convolve_workspace_bytes", "flanhip_convolve", "flanhip_convolve_dev",
                "flanhip_convolve_debug_partition"]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _formula(ch, n, irch, m, P):
    K, J = -(-m // P), -(-(n + m) // P)
    return 8 * (P + 1) * (2 * ch * J + min(ch, irch) * K) + 8192


def test_convolve_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    for name in CONV_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name


def test_out_frames_is_n_plus_m():
    assert fa.convolve_out_frames(1, 1) == 2
    assert fa.convolve_out_frames(2_880_000, 144_000) == 3_024_000
    assert fa.convolve_out_frames(3_000_000_000, 5) == 3_000_000_005          # 64-bit
    assert fa.convolve_out_frames(0, 5) == 0 and fa.convolve_out_frames(5, -1) == 0


@pytest.mark.parametrize("n,m,P", [(1, 1, 512), (48000, 16384, 512), (48000, 16385, 1024), (2_880_000, 144_000, 8192 // 2),
                                   (2_880_000, 24_000, 1024), (480_000, 480_000, 4096), (10, 10_000_000, 4096)])
def test_partition_rule(n, m, P):
    assert fa.convolve_partition(n, m) == P


@pytest.mark.parametrize("ch,n,irch,m", [(1, 1, 1, 1), (2, 2_880_000, 2, 144_000), (8, 2_880_000, 1, 24_000), (1, 480_000, 1, 480_000),
                                         (1, 100, 2, 5000), (3, 777, 2, 100_000)])
def test_workspace_bytes_follow_the_formula(ch, n, irch, m):
    assert fa.convolve_workspace_bytes(ch, n, irch, m) == _formula(ch, n, irch, m, fa.convolve_partition(n, m))


def test_workspace_bytes_under_a_forced_partition():
    for P in (128, 256, 512, 1024, 2048, 4096):
        with fa.convolve_partition_forced(P):
            assert fa.convolve_workspace_bytes(2, 10_000, 1, 3000) == _formula(2, 10_000, 1, 3000, P)
    for bad in (64, 1000, 8192):
        with fa.convolve_partition_forced(bad):
            assert fa.convolve_workspace_bytes(2, 10_000, 1, 3000) == 0
    assert fa.convolve_workspace_bytes(2, 10_000, 1, 3000) == _formula(2, 10_000, 1, 3000, 512)     # back to the library's choice


def test_workspace_bytes_refusals():
    assert fa.convolve_workspace_bytes(0, 100, 1, 10) == 0
    assert fa.convolve_workspace_bytes(1, 0, 1, 10) == 0
    assert fa.convolve_workspace_bytes(1, 100, 0, 10) == 0
    assert fa.convolve_workspace_bytes(1, 100, 1, -3) == 0


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((1, 100), np.float32)
    h = np.zeros((1, 10), np.float32)
    out = np.zeros((1, 110), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    assert L.flanhip_convolve(None, 1, 100, p(h), 1, 10, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, 100, None, 1, 10, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, 100, p(h), 1, 10, 48000.0, 1, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 0, 100, p(h), 1, 10, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, -1, p(h), 1, 10, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, 100, p(h), 0, 10, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, 100, p(h), 1, 0, 48000.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve(p(x), 1, 100, p(h), 1, 10, 0.0, 1, p(out), None) == fa.ERR_INVALID_ARG
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    assert L.flanhip_convolve_dev(None, 1, 100, ws, 1, 10, 48000.0, 0, ws, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve_dev(ws, 1, 100, ws, 1, 10, 48000.0, 0, ws, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_convolve_dev(ws, 1, 100, ws, 1, 0, 48000.0, 0, ws, ws, None) == fa.ERR_INVALID_ARG
    with fa.convolve_partition_forced(300):
        assert L.flanhip_convolve(p(x), 1, 100, p(h), 1, 10, 48000.0, 1, p(out), None) == fa.ERR_UNSUPPORTED


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    x = np.ones((1, 100), np.float32)
    h = np.ones((1, 10), np.float32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.convolve(x, h, 48000.0)
    assert e.value.code == fa.ERR_NO_DEVICE
