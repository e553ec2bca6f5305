"""The C++ Audio::filter_1pole_multinotch / filter_2pole_multinotch (include/flan/Audio.h over libflan_host.so), driven by
tests/cpp/multinotch_test.cpp: null in, null out; the saturator, order 0 and an over-large order each a message and a null Audio (and, without a
device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null result, nothing sampled); on a device, each method with constants
and with callables against the C ABI's host form fed what the method samples, bit for bit."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("multinotch_test")


def test_multinotch_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_multinotch_methods_on_device():
    _build()
    _run("--device")
