"""The C++ Audio::synthesize_spectrum (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/spectrum_test.cpp: every invalid argument of
AudioSynthesis.cpp:163-168 gives a null Audio; a size the library does not serve gives a null Audio and a line on stderr; without a device a
valid call gives a null Audio, loudly; on a device the method with explicit phases equals flanhip_audio_synthesize_spectrum on the same
arrays bit for bit (a one-workgroup and a two-pass table, a swept frequency, the sd <= 0.001 branch), and with random phases two calls differ
and each is normalised.  tests/test_gpu_spectrum.py holds the values to the truth and to the reference-made vectors."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("spectrum_test")


def test_spectrum_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failures are reported, not silent
    assert "synthesize_spectrum refused" in r.stderr


@pytest.mark.gpu
def test_spectrum_on_device():
    _build()
    _run("--device")
