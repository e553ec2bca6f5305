"""The C++ Audio::ring_modulate, fade / fade_frames, invert_phase, waveshape, add_moisture, apply_adsr_envelope, apply_ar_envelope,
get_total_energy, get_energy_difference, get_amplitude_envelope, synthesize_waveform and synthesize_white_noise, with flan::ADSR and
flan::Waveform (include/flan/Audio.h, include/flan/Function.h over libflan_host.so), driven by tests/cpp/volume_test.cpp: null inputs, the
host-side decisions, the ADSR anchors and the named waveforms as host functions without a device, where every method fails loudly with a null
Audio; on a device every method against the composition of public pieces it is defined as, bit for bit.  The methods' results against the
restatement are tests/test_gpu_volume.py's."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("volume_test")


def test_volume_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failures are reported, not silent


@pytest.mark.gpu
def test_volume_methods_on_device():
    _build()
    r = _run("--device")
    assert "volume methods on the device" in r.stdout
