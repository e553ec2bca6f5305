"""The C++ Audio::filter_2pole_lowpass, _bandpass, _highpass, _notch, filter_2pole_lowshelf, _bandshelf, _highshelf and filter_1pole_lowshelf,
_highshelf (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/filter2_test.cpp: null in, null out (and, without a device,
FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null result); on a device, every method with constants and with callables
against the C ABI bit for bit, the notch against the band-pass, the times the 2-pole shelves sample at, and order 0."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("filter2_test")


def test_filter2_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_filter2_methods_on_device():
    _build()
    _run("--device")
