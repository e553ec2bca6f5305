"""The C++ Audio::filter_1pole_multinotch / filter_2pole_multinotch (include/flan/Audio.h over libflan_host.so), driven by
tests/cpp/multinotch_test.cpp: null in, null out; the saturator, order 0 and an over-large order each a message and a null Audio (and, without a
device, FLANHIP_ERR_NO_DEVICE from the C ABI and a loud failure with a null result, nothing sampled); on a device, each method with constants
and with callables against the C ABI's host form fed what the method samples, bit for bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "multinotch_test")


def _build():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "flan_amd", "host")], check=True)
    src = os.path.join(ROOT, "tests", "cpp", "multinotch_test.cpp")
    deps = [src, os.path.join(ROOT, "flan_amd", "libflan_host.so")]
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), src, "-o", BIN,
                        "-L" + os.path.join(ROOT, "flan_amd"), "-lflan_host", "-lflanhip",
                        "-Wl,-rpath," + os.path.join(ROOT, "flan_amd"), "-lpthread"], check=True)


def _run(*args):
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "flan_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([BIN] + list(args), capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
    return r


def test_multinotch_host_checks_without_a_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run("--no-device")
    assert "flan:" in r.stderr                                           # the failure is reported, not silent


@pytest.mark.gpu
def test_multinotch_methods_on_device():
    _build()
    _run("--device")
