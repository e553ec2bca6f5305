"""The C++ Audio::get_loud_chunks, remove_silence, remove_edge_silence, reverse, modify_boundaries, the splits, rearrange, random_chunks, iterate
and delay (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/temporal_test.cpp: null inputs and the host-side decisions without a
device, where every method fails loudly with a null Audio; on a device the method surface -- fused against general paths, seeds, nothing noisy.
The methods' results against the restatement are tests/test_gpu_temporal.py's."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("temporal_test")


def test_temporal_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failures are reported, not silent


@pytest.mark.gpu
def test_temporal_methods_on_device():
    _build()
    r = _run("--device")
    assert "temporal methods on the device" in r.stdout
