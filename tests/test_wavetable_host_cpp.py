"""The C++ flan::Wavetable (include/flan/Wavetable.h over libflan_host.so), driven by tests/cpp/wavetable_test.cpp: null sources and bad
arguments; without a device both constructors give a null Wavetable, loudly, and synthesize a null Audio; on a device, construction in the
three pitch modes from a 0.25 s 220 Hz tone, get_num_waveforms, the table against the C ABI bit for bit, synthesis at the tone's own
frequency (the spectrum's peak within one bin of 220 Hz), the four edits and the functional constructor.  tests/test_gpu_wavetable.py holds
the values to the truth and to the reference-made vectors."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("wavetable_test")


def test_wavetable_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failures are reported, not silent


@pytest.mark.gpu
def test_wavetable_on_device():
    _build()
    _run("--device")
