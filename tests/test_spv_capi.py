"""The sliding-DFT vocoder's C ABI (include/flanhip.h, flan_amd/csrc/spv.hip) without a device: symbols, host arithmetic, refusals."""
import ctypes
import os

import numpy as np
import pytest

import spv_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPV_SYMBOLS = ["flanhip_spv_analyze", "flanhip_spv_analyze_dev", "flanhip_spv_synthesize_workspace_bytes", "flanhip_spv_synthesize",
               "flanhip_spv_synthesize_dev", "flanhip_spv_modify_frequency_const_dev", "flanhip_spv_twiddles",
               "flanhip_spv_debug_chain_length"]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_spv_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    for name in SPV_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name


def test_workspace_bytes_without_a_device():
    ws = fa.spv_synthesize_workspace_bytes(2, 48000, 1024, 48000.0)
    assert ws > 0 and ws % (8 * 2 * 1024) == 0
    assert fa.spv_synthesize_workspace_bytes(1, 100, 1, 48000.0) == 0          # N < 2
    assert fa.spv_synthesize_workspace_bytes(0, 100, 64, 48000.0) == 0
    assert fa.spv_synthesize_workspace_bytes(1, 0, 64, 48000.0) == 0
    # the debug cut changes the chain count, and the size with it
    with fa.spv_chain_length(10):
        assert fa.spv_synthesize_workspace_bytes(1, 1000, 64, 48000.0) == 2 * 8 * 100 * 64          # a total and a peak per chain and bin


def test_twiddles_are_the_restatements_to_the_bit():
    for N in (2, 3, 7, 100, 1024, 4096):
        got = fa.spv_twiddles(N)
        re, im = R.twiddles(N)
        assert np.array_equal(got[:, 0].view(np.uint32), re.view(np.uint32)), N
        assert np.array_equal(got[:, 1].view(np.uint32), im.view(np.uint32)), N


def test_fewer_than_two_bins_is_unsupported():
    x = np.zeros((1, 16), np.float32)
    for N in (1, 0, -3):
        with pytest.raises(fa.FlanHipError) as e:
            fa.spv_analyze(x, 48000.0, N) if N > 0 else fa.check(fa.lib.flanhip_spv_analyze(fa._ptr(x), 1, 16, 48000.0, N, fa._ptr(x), None))
        assert e.value.code == fa.ERR_UNSUPPORTED
    spv = np.zeros((1, 16, 1, 2), np.float32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.spv_synthesize(spv, 48000.0)
    assert e.value.code == fa.ERR_UNSUPPORTED
    with pytest.raises(fa.FlanHipError) as e:
        fa.spv_twiddles(1)
    assert e.value.code == fa.ERR_UNSUPPORTED


def test_compute_calls_fail_loudly_without_a_device():
    if not _no_gpu():
        pytest.skip("GPU visible")
    x = np.zeros((1, 256), np.float32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.spv_analyze(x, 48000.0, 64)
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.spv_synthesize(np.zeros((1, 256, 64, 2), np.float32), 48000.0)
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.spv_modify_frequency_const_dev(0x1000, 1, 256, 64, 1.0, 0, 0x1000)
    assert e.value.code == fa.ERR_NO_DEVICE
