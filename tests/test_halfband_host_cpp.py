"""The C++ Audio::halfband_modulate, shift_frequency and halfband_multiply (include/flan/Audio.h over libflan_host.so), driven by
tests/cpp/halfband_test.cpp: null in, null out (and, without a device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null
result, nothing sampled); on a device, every method with constants and with callables against the C ABI fed what the method computes on
the host, bit for bit."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("halfband_test")


def test_halfband_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_halfband_methods_on_device():
    _build()
    _run("--device")
