"""The C++ drop-in surface (include/flan/*.h over libflan_host.so + libflanhip.so), driven by tests/cpp/host_test.cpp."""
import pytest

import host_cpp

# (this driver alone is compiled with the compiler's default floating-point contraction, and its tests do the checking themselves)
BIN, _build, _run_args = host_cpp.driver("host_test", check=False, timeout=300, fp_contract_off=False)


def _run(args):
    return _run_args(*args)


def test_host_surface_without_device(tmp_path):
    """no GPU: null objects and a loud error, never a CPU fallback"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    _build()
    r = _run(["--no-device", "--flan-file=%s" % (tmp_path / "host_test.flan")])
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout


@pytest.mark.gpu
def test_host_surface_on_device():
    _build()
    r = _run([])
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASSED" in r.stdout
