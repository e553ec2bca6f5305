"""The C++ Audio::filter_1pole_lowpass, _highpass, _split, _repeat_low and _repeat_high (include/flan/Audio.h over libflan_host.so), driven
by tests/cpp/filter_test.cpp: null in, null out (and, without a device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null
result); on a device, every method with a constant and a callable cutoff against the C ABI bit for bit, split against the compositions it
stands for, order 0 and no repeats, and a chain from convert_to_PV through filter_1pole_highpass to set_volume that stays in HBM."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("filter_test")


def test_filter_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_filter_methods_on_device():
    _build()
    _run("--device")
