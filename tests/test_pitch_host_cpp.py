"""The C++ Audio::get_local_wavelength(s), get_average_wavelength, get_local_frequency / frequencies and get_frequency_envelope
(include/flan/Audio.h over libflan_host.so), driven by tests/cpp/pitch_test.cpp: a null Audio's answers; without a device
FLANHIP_ERR_NO_DEVICE from the C ABI and loud failures with empty answers, while the host-only parts work; on a device, the methods against
the C ABI's host form on the same samples, bit for bit.  tests/test_gpu_pitch.py holds the methods' values to the truth."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("pitch_test")


def test_pitch_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failures are reported, not silent


@pytest.mark.gpu
def test_pitch_methods_on_device():
    _build()
    _run("--device")
