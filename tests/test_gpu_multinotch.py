"""Audio::filter_1pole_multinotch / filter_2pole_multinotch on the MI355X (flan_amd/csrc/multinotch.hip) against the NumPy restatement
(tests/multinotch_reference.py) on its case table: the truth criterion (the device's distance from the fp64 truth at most 4 x the fp32
loop's own, or 8 fp32 ulps of the output's peak) and the bounds against the fp32 loop (multinotch_reference.REL_RMS_BOUND / REL_MAX_BOUND per
kind of input, divided by the rms and the peak of the INPUT; measured values: DESIGN.md 4.19).  Every figure is printed before it is held."""
import ctypes

import numpy as np
import pytest
import torch

import flan_amd as fa
import multinotch_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def params(c):
    return c["cutoff"], c["damping"], c["feedback"], c["wet_dry"]


def run(c, x=None, frames=None):
    with fa.multinotch_run_forced(c["run"] if frames is None else frames):
        return fa.multinotch(c["x"] if x is None else x, c["sr"], *params(c), kind=c["kind"], order=c["order"], invert=c["invert"])


def to_dev(v):
    return torch.from_numpy(np.array(v, F32)).to(torch.device("cuda", 0))      # a copy: the cases are read-only


def run_dev(c, alias=False):
    """the _dev form with its workspace filled with 0xFF and its output with NaN beforehand"""
    dev = torch.device("cuda", 0)
    ch, n = c["x"].shape
    with fa.multinotch_run_forced(c["run"]):
        d_x = to_dev(c["x"])
        d_out = d_x if alias else torch.full((ch, n), float("nan"), dtype=torch.float32, device=dev)
        d_ws = torch.full((fa.multinotch_workspace_bytes(ch, n, c["kind"], c["order"]),), 0xFF, dtype=torch.uint8, device=dev)
        keep = [v if np.isscalar(v) else to_dev(v) for v in params(c)]
        fa.multinotch_dev(d_x, ch, n, c["sr"], *keep, c["kind"], c["order"], c["invert"], d_out, d_ws)
        torch.cuda.synchronize()
    return d_out.cpu().numpy()


def held(name, got, what=""):
    """prints the case's figures, then returns what it misses"""
    c, e = R.case(name), R.expected(name)
    rms_x, peak_x = R.input_scale(c["x"])
    rms, mx = R.errors(got, e["y32"])
    rel_rms, rel_max = rms / rms_x, mx / peak_x
    ok, (t_rms, t_max, own_rms, own_max, floor) = R.truth_criterion(got, e["y32"], e["y64"])
    differ = int(np.count_nonzero(got.view(np.uint32) != e["y32"].view(np.uint32)))
    print("%s%s [%s]: vs restatement rel_rms=%.3e rel_max=%.3e (%d of %d differ); vs truth rms=%.3e max=%.3e (the restatement: %.3e, %.3e; floor %.3e)"
          % (name, what, c["input"], rel_rms, rel_max, differ, got.size, t_rms, t_max, own_rms, own_max, floor))
    missed = []
    if not np.all(np.isfinite(got)):
        missed.append("not finite")
    if not ok:
        missed.append(("truth", t_rms, t_max, own_rms, own_max, floor))
    if not (rel_rms <= R.REL_RMS_BOUND[c["input"]] and rel_max <= R.REL_MAX_BOUND[c["input"]]):
        missed.append(("restatement", rel_rms, rel_max))
    return missed


@pytest.mark.parametrize("name", R.IDS)
def test_against_the_restatement_and_the_truth(name):
    got = run(R.case(name))
    assert got.dtype == F32 and got.shape == R.case(name)["x"].shape
    missed = held(name, got)
    assert not missed, missed


@pytest.mark.parametrize("name", ["p1_o2_n3", "p1_o16_n1000", "p1_o8_n8192", "p2_o3_n255", "p2_o4_n8192", "p2_o8_n9001"])
def test_host_and_device_forms_and_two_calls_are_bit_identical(name):
    c = R.case(name)
    host = run(c)
    assert R.same_bits(run_dev(c), host)
    assert R.same_bits(run(c), host)
    assert R.same_bits(run_dev(c, alias=True), host)              # out aliasing the input


@pytest.mark.parametrize("name", ["p1_o16_n1000", "p1_o8_n8192", "p2_o3_n255", "p2_o4_n8192"])
def test_a_channel_does_not_depend_on_its_neighbours(name):
    c = R.case(name)
    assert c["x"].shape[0] == 3
    whole = run(c)
    for channel in range(3):
        assert R.same_bits(run(c, x=c["x"][channel:channel + 1]), whole[channel:channel + 1])
    assert R.same_bits(run(c, x=c["x"][::-1])[::-1], whole)


@pytest.mark.parametrize("name", R.LONG_NOISE)
def test_forced_runs_stay_within_the_bounds(name):
    c = R.case(name)
    missed = []
    for frames in (1, 4, 16, 64):
        missed += held(name, run(c, frames=frames), " run %d" % frames)
    assert not missed, missed


@pytest.mark.parametrize("kind,order,n", [(R.ONE_POLE, 2, 2100), (R.ONE_POLE, 7, 1100), (R.TWO_POLE, 8, 1100)])
def test_the_carry_goes_past_one_pass_of_its_width(kind, order, n):
    """k_mn_carry scans 128 / DP block totals in a pass (32, 16, 8 for DP = 4, 8, 16), and at run 1 a block is as many frames: 2100 frames are
    66 blocks and 3 passes at DP = 4, 1100 frames 69 blocks and 5 passes at DP = 8, 138 blocks and 18 passes at DP = 16.  The last pass is
    ragged every time.  Held to the truth criterion from the state every pass hands the next"""
    x = R.signal("noise", 2, n, np.random.default_rng(99))
    cutoff, damping, feedback, wet_dry = R.curves(n)
    y32, _ = R.multinotch(x, 48000.0, kind, order, cutoff, damping, feedback, wet_dry, True, dtype=F32)
    y64, _ = R.multinotch(x, 48000.0, kind, order, cutoff, damping, feedback, wet_dry, True, dtype=F64)
    with fa.multinotch_run_forced(1):
        got = fa.multinotch(x, 48000.0, cutoff, damping, feedback, wet_dry, kind=kind, order=order, invert=True)
    ok, figures = R.truth_criterion(got, y32, y64)
    print("carry kind %d order %d: t_rms=%.3e t_max=%.3e own_rms=%.3e own_max=%.3e floor=%.3e" % ((kind, order) + figures))
    assert np.all(np.isfinite(got)) and ok, figures
    # the tail, which only the later passes reach, on its own
    ok_tail, figures = R.truth_criterion(got[:, n - 64:], y32[:, n - 64:], y64[:, n - 64:])
    assert ok_tail, figures


@pytest.mark.parametrize("name,m", [("p1_o16_n1000", 333), ("p2_o4_n8192", 5000), ("p1_o3_n9001", 8999)])
def test_causality(name, m):
    """changing frames >= m leaves frames < m bit for bit"""
    c = R.case(name)
    x = c["x"].copy()
    x[:, m:] = np.random.default_rng(5).normal(0.0, 0.5, x[:, m:].shape).astype(F32)
    before, after = run(c), run(c, x=x)
    assert R.same_bits(after[:, :m], before[:, :m]) and not R.same_bits(after[:, m:], before[:, m:])


@pytest.mark.parametrize("name,m", [("p1_o16_n1000", 500), ("p2_o4_n8192", 4100)])
def test_a_nan_sample_stays_in_its_channel_and_its_future(name, m):
    c = R.case(name)
    assert c["x"].shape[0] == 3
    x = c["x"].copy()
    x[1, m] = np.nan
    clean, got = run(c), run(c, x=x)
    assert R.same_bits(got[0:1], clean[0:1]) and R.same_bits(got[2:3], clean[2:3])
    assert R.same_bits(got[1:2, :m], clean[1:2, :m])
    assert not np.isfinite(got[1, m])


def test_cancel_and_curves_through_the_c_abi():
    c = R.case("p2_o4_n8192")
    flag = ctypes.c_int(1)
    with pytest.raises(fa.FlanHipError) as e:
        fa.multinotch(c["x"], c["sr"], *params(c), kind=c["kind"], order=c["order"], invert=c["invert"], cancel=flag)
    assert e.value.code == fa.ERR_CANCELLED
    flag.value = 0
    got = fa.multinotch(c["x"], c["sr"], *params(c), kind=c["kind"], order=c["order"], invert=c["invert"], cancel=flag)
    assert R.same_bits(got, run(c))
