"""The C++ Audio::stereo_spatialize, pan / pan_in_place / widen, convert_to_stereo / convert_to_mono and combine_channels / split_channels
(include/flan/Audio.h over libflan_host.so), driven by tests/cpp/spatial_test.cpp: null in, null out; a non-mono input of
stereo_spatialize refused with the reference's message; a moving source on 32 frames or fewer a null Audio and one line (and, without a
device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null result, nothing sampled); on a device, stereo_spatialize with a
constant position (the pure delay and its length) and with a callable orbit against the C ABI's host forms fed what the method samples, bit
for bit, and pan, widen, the conversions and the channel copies against host loops, bit for bit."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("spatial_test")


def test_spatial_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_spatial_methods_on_device():
    _build()
    _run("--device")
