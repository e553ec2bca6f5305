"""The C++ Audio::filter_comb (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/comb_test.cpp: null in, null out (and, without
a device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null result, nothing sampled); on a device, the method with
constants and with callables against the C ABI's host form fed what the method samples, bit for bit."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("comb_test")


def test_comb_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_comb_method_on_device():
    _build()
    _run("--device")
