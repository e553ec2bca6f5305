"""Every frame processor of the C++ flan::PV surface (include/flan/PV.h over flan_amd/host/PV.cpp), its whole output against the oracle.

tests/cpp/pv_methods_test.cpp runs once, in a child process, on seeded inputs written here; it calls each method with callables and
constants and writes every result out.  tests/pv_methods_reference.py restates the callables in NumPy float32, the length rules from the
reference lines PV.cpp cites, and computes what each case must give with tests/oracle_lib.py.  One test per case: the format fields, then
the bits -- except a sampled resonate decay (the criterion of test_gpu_processors_ext.py::test_resonate_decay_grid: the device rounds pow
correctly, libm does not promise to) and convert_to_audio (the bound of test_gpu_conversions.py::test_synthesis_parity, rms <= 1e-5,
against the oracle's synthesis of the PV the driver wrote)."""
import os
import time

import numpy as np
import pytest

import oracle_lib as O
import pv_methods_reference as R
from test_pv_methods_reference import build_driver, run_driver, sample_only

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    build_driver()
    in_dir, out_dir = tmp_path_factory.mktemp("pv_methods_in"), tmp_path_factory.mktemp("pv_methods_out")
    for name, data in R.inputs().items():
        R.write_pv(os.path.join(str(in_dir), name + ".pv"), R.FORMATS[name], data)
    dumps = sample_only(tmp_path_factory.mktemp("pv_methods_samples"))
    t0 = time.time()
    r = run_driver("--run", str(in_dir), str(out_dir), timeout=240)
    print("\n[pv_methods_test --run] %.1f s\n%s%s" % (time.time() - t0, r.stdout, r.stderr))
    return dict(returncode=r.returncode, output=r.stdout + r.stderr, out_dir=str(out_dir), dumps=dumps)


def test_driver_ran(driver):
    """one failure, with the driver's output, when it exits non-zero (its own checks: the input's bits after every case; device-only
    against host-current inputs of the data-dependent methods)"""
    assert driver["returncode"] == 0 and "PASSED" in driver["output"], driver["output"]


def _result(driver, name):
    path = os.path.join(driver["out_dir"], name + ".pv")
    if driver["returncode"] != 0 and not os.path.exists(path):
        pytest.fail("the driver failed before this case (see test_driver_ran)", pytrace=False)
    assert os.path.exists(path), "the driver wrote no " + name
    return R.read_pv(path)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _check_format(name, fields, fmt):
    if fmt is None:
        assert fields == R.NULL_FIELDS, "%s: a null result expected, got %r" % (name, fields)
    else:
        assert fields == fmt.fields(), "%s: format %r, expected %r" % (name, fields, fmt.fields())


_expected = {}


def _expect(case, driver):
    if case.name not in _expected:
        ins = R.inputs()
        _expected[case.name] = case.expect(ins, driver["dumps"]) if getattr(case.expect, "needs_dumps", False) else case.expect(ins)
    return _expected[case.name]


@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_case(driver, case):
    assert ("case %s:" % case.name) in driver["output"], "the driver printed no line for this case"
    if case.how == "audio_rms":
        fields, audio = _result(driver, case.name)
        src_fields, pv = (R.FORMATS[case.inp].fields(), R.inputs()[case.inp]) if case.source is None else _result(driver, case.source)
        assert audio is not None and pv is not None
        ch, frames, bins, window, sr, ar = src_fields
        ref, flag = O.synthesize(pv, sr, ar, window)
        assert flag == 0
        assert fields == (ch, ref.shape[1], 0, 0, sr, 0.0) and audio.shape == ref.shape
        rms = float(np.sqrt(np.mean((audio.astype(np.float64) - ref.astype(np.float64)) ** 2)))
        print("\n[%s] rms diff=%.3e (signal rms %.3e)" % (case.name, rms, float(np.sqrt(np.mean(ref.astype(np.float64) ** 2)))))
        assert rms <= 1e-5
        return
    want = _expect(case, driver)
    if "#count" in want:                                                    # split_at_times: that many pieces, no more
        assert ("case %s: %d pieces" % (case.name, want["#count"])) in driver["output"]
        assert not os.path.exists(os.path.join(driver["out_dir"], "%s#%d.pv" % (case.name, want["#count"])))
    if case.how == "resonate_grid":
        fields, got = _result(driver, case.name)
        fmt, libm = want[""]
        exact = want["#exact"][1]
        _check_format(case.name, fields, fmt)
        same = float(np.mean(_bits(got) == _bits(exact)))
        d = np.abs(got[..., 0].astype(np.float64) - libm[..., 0]).max() / np.abs(libm[..., 0]).max()
        print("\n[%s] bit-identical to correctly rounded pow: %.6f; max |dm| vs libm powf, relative to max m: %.2e" % (case.name, same, d))
        assert same >= 0.9999
        assert d <= 1e-5
        return
    for suffix, value in want.items():
        if suffix in ("#count", "#exact"):
            continue
        fmt, ref = value
        fields, got = _result(driver, case.name + suffix)
        _check_format(case.name + suffix, fields, fmt)
        if ref is not None:
            differ = int(np.any(_bits(got) != _bits(ref), axis=-1).sum())
            assert differ == 0, "%s: %d of %d MFs differ in their bits" % (case.name + suffix, differ, ref.size // 2)
