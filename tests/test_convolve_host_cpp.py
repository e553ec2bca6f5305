"""The C++ Audio::convolve (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/convolve_test.cpp: null objects (and,
without a device, a loud failure with a null result), and on a device the C ABI, the resample rule and the normalize gain bit for bit."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("convolve_test")


def test_convolve_without_a_device_is_null_and_loud():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_convolve_equals_the_c_abi_on_device():
    _build()
    _run("--device")
