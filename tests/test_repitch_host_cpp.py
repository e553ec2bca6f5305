"""The C++ Audio::repitch (include/flan/Audio.h over libflan_host.so), driven by tests/cpp/repitch_test.cpp: null input, the Linear
answer (and, without a device, a loud failure with a null result); on a device, cases of the reference-made fixture through
Audio::repitch from the factors before inversion -- 0, negative and 1e-6 among them, so the method's own clamp is what is checked --
against the C ABI bit for bit and the reference-made output, a ramp for the Function sampling, and the length of a constant Function."""
import struct

import numpy as np
import pytest

import host_cpp
import repitch_reference as R

BIN, _build, _run = host_cpp.driver("repitch_test")
FIXTURE_CASES = ("up1p5", "step", "u_down0p7", "zero", "negative", "tiny")
# the factors of the clamp cases before inversion (golden/ref_made/make_wdl_repitch.py); the fixture keeps only what the clamp made of them
RAW_FACTORS = {"zero": 0.0, "negative": -2.0, "tiny": 1e-6}


def _write_fixture(path):
    cases = [c for c in R.load_cases() if c["name"] in FIXTURE_CASES]
    assert len(cases) == len(FIXTURE_CASES)
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            ch, n = c["x"].shape
            f.write(struct.pack("<6if", ch, n, c["g"], c["quality"], c["inv"].size, c["out_frames"], c["sr"]))
            f.write(np.ascontiguousarray(c["x"], "<f4").tobytes())
            inv = np.ascontiguousarray(c["inv"], "<f4")
            if c["name"] in RAW_FACTORS:
                factors = np.full(inv.size, RAW_FACTORS[c["name"]], "<f4")
            else:
                factors = (np.float32(1) / inv).astype("<f4")
                assert np.array_equal(np.float32(1) / factors, inv)          # the round trip through 1 / v is exact for these cases
            f.write(factors.tobytes())
            f.write(inv.tobytes())
            f.write(np.ascontiguousarray(c["out"], "<f4").tobytes())


def test_repitch_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_repitch_equals_the_c_abi_on_device(tmp_path):
    _build()
    path = str(tmp_path / "repitch_cases.bin")
    _write_fixture(path)
    _run("--device", path)
