"""The C++ sliding-DFT surface (include/flan/SPV.h, SPVBuffer.h, Audio::convert_to_SPV over libflan_host.so), driven by
tests/cpp/spv_test.cpp: format arithmetic without a device, null objects without one, and the classes against the C ABI on one."""
import pytest

import host_cpp

BIN, _build, _run = host_cpp.driver("spv_test")


def test_spv_format_arithmetic_and_buffer_positions():
    _build()
    _run("--host")


def test_spv_conversions_without_a_device_are_null():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    _run("--no-device")


@pytest.mark.gpu
def test_spv_classes_equal_the_c_abi_on_device():
    _build()
    _run("--device")
