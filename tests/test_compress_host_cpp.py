"""The C++ Audio::compress, modify_volume and set_volume (include/flan/Audio.h over libflan_host.so), driven by
tests/cpp/compress_test.cpp: null in, null out, the short and the null sidechain (and, without a device, FLANHIP_ERR_NO_DEVICE from the C ABI
and a loud failure with a null result); on a device, the three methods with constant and callable Functions against the C ABI and the
reference's host arithmetic bit for bit, the in-place forms, and a chain from convert_to_PV to set_volume that stays in HBM."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("compress_test")


def test_compress_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_compress_methods_on_device():
    _build()
    _run("--device")
