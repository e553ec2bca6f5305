"""Audio::filter_2pole_lowpass / _bandpass / _highpass / _notch, filter_2pole_lowshelf / _bandshelf / _highshelf and filter_1pole_lowshelf /
_highshelf on the MI355X (flan_amd/csrc/filter.hip) against the NumPy restatement (tests/filter2_reference.py): the fp32 loop and the fp64
truth.  Errors are divided by the rms and the peak of the INPUT.  The bounds (filter2_reference.REL_RMS_BOUND, REL_MAX_BOUND) and the
measured values they are set from (<= 30 % above): DESIGN.md 4.16."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import filter2_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
REL_RMS_BOUND, REL_MAX_BOUND, TRUTH_FACTOR, TRUTH_FLOOR = R.REL_RMS_BOUND, R.REL_MAX_BOUND, R.TRUTH_FACTOR, R.TRUTH_FLOOR
# the cases whose length is a multiple of 4, over one block and over three, 2 and 3 channels: there (and only there) the kernels read and
# write 16 bytes at a time, so every property below is held on them as well
QUADS = tuple(c["name"] for c in R.CASES if c["cls"] == R.PARITY and c["x"].shape[1] % 4 == 0 and c["x"].shape[1] >= R.BLOCK)
assert len(QUADS) == 8
NO_NOTCH_QUADS = tuple(q for q in QUADS if R.case(q)["kind"] != R.NOTCH)


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def run(c, x=None):
    return fa.filter2(c["x"] if x is None else x, c["sr"], c["cutoff"], c["damping"], c["gain"], kind=c["kind"], order=c["order"])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def to_dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, F32)).to(torch.device("cuda", 0))


def run_dev(c, alias=False):
    """the _dev form with its workspace filled with 0xFF and its output with NaN beforehand"""
    dev = torch.device("cuda", 0)
    ch, n = c["x"].shape
    d_x = to_dev(c["x"])
    d_out = d_x if alias else torch.full((ch, n), float("nan"), dtype=torch.float32, device=dev)
    d_ws = torch.full((fa.filter2_workspace_bytes(ch, n),), 0xFF, dtype=torch.uint8, device=dev)
    args = [v if np.isscalar(v) else to_dev(v) for v in (c["cutoff"], c["damping"], c["gain"])]
    fa.filter2_dev(d_x, ch, n, c["sr"], *args, c["kind"], c["order"], d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("name", R.CHECKED_IDS)
def test_against_the_restatement_and_the_truth(name):
    """parity cases: the absolute bounds against the fp32 restatement AND the truth criterion; truth_only cases (fixed by name in
    filter2_reference.TRUTH_ONLY_NAMES): the truth criterion alone"""
    c = R.case(name)
    got = run(c)
    want, truth = R.expected(name, F32), R.expected(name, F64)
    assert got.shape == want.shape and got.dtype == F32
    rel_rms, rel_max = R.errors(got, want, c["x"])
    t_rms, t_max = R.errors(got, truth, c["x"])
    own_rms, own_max = R.errors(want, truth, c["x"])
    differ = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    print("%s (%s): vs restatement rel_rms=%.3e rel_max=%.3e (%d of %d differ); vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
          % (name, c["cls"], rel_rms, rel_max, differ, got.size, t_rms, t_max, own_rms, own_max))
    failures = []
    if c["cls"] == R.PARITY and not (rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND):
        failures.append(("restatement", rel_rms, rel_max))
    if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
        failures.append(("truth", t_rms, t_max, own_rms, own_max))
    assert not failures, failures


def test_host_and_device_forms_are_bit_identical():
    for name in ("low4_1k_d07_p6", "high3_1k_dcurve_gcurve", "notch3_wobble_d025_gcurve", "bandshelf2_wobble_dover_m12", "shelf1high1_wobble_dcurve_m12",
                 "shelf1low3", "n1_low3", "n4095_lowshelf3") + QUADS:
        c = R.case(name)
        assert same_bits(run(c), run_dev(c)), name


def test_out_may_alias_the_input_but_not_for_the_notch():
    for name in ("low3_wobble_dcurve_m12", "band4_wobble_dcurve_m12", "highshelf4_1k_d025_p6", "shelf1low1_sweep_dcurve_p6", "n1025_bandshelf2",
                 "lowshelf0_sweep_d07_m12", "shelf1high0_sweep_d07_m12") + NO_NOTCH_QUADS:
        c = R.case(name)
        assert same_bits(run_dev(c), run_dev(c, alias=True)), name
    for name in ("notch0_wobble_dover_m12", "notch3_wobble_d025_gcurve", "n12304_notch2_mixed"):
        c = R.case(name)
        x = c["x"].copy()
        with pytest.raises(fa.FlanHipError) as e:
            run_dev(c, alias=True)
        assert e.value.code == fa.ERR_INVALID_ARG and "aliases" in str(e.value), name
        assert same_bits(c["x"], x)


def test_two_runs_are_bit_identical():
    for name in ("high4_sweep_d025_m12", "lowshelf3_sweep_dcurve_p6", "shelf1high3"):
        assert same_bits(run(R.case(name)), run(R.case(name))), name


def test_a_channel_does_not_depend_on_the_channels_filtered_with_it():
    for name in ("low3_wobble_dcurve_m12", "notch3_wobble_d025_gcurve", "shelf1low2") + QUADS:
        c = R.case(name)
        out = run(c)
        assert c["x"].shape[0] > 1, name
        for k in range(c["x"].shape[0]):
            assert same_bits(run(c, c["x"][k:k + 1])[0], out[k]), (name, k)


@pytest.mark.parametrize("frames", [1, 7, 64])
def test_the_run_length_changes_nothing_beyond_rounding(frames):
    """7: runs that do not start on 16-byte boundaries (the scalar loads); 1: 49 blocks a channel for 12 305 frames; 64: one, and with
    the lengths that are multiples of 4 the 16-byte loads over runs of 16 quads"""
    for name in ("high4_sweep_d025_m12", "highshelf3_wobble_dcurve_m12", "shelf1high1_wobble_dcurve_m12") + QUADS:
        c = R.case(name)
        assert c["cls"] == R.PARITY
        out = run(c)
        with fa.filter_run_forced(frames):
            out_f = run(c)
        for what, want in (("the default run", out), ("the restatement", R.expected(name, F32))):
            rel_rms, rel_max = R.errors(out_f, want, c["x"])
            print("%s run %d vs %s: rel_rms=%.3e rel_max=%.3e" % (name, frames, what, rel_rms, rel_max))
            assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (name, what)


def test_later_input_does_not_reach_earlier_output():
    """a carry taken from an inclusive total would"""
    for name in ("low3_wobble_dcurve_m12", "highshelf4_1k_d025_p6", "shelf1high1_wobble_dcurve_m12") + tuple(q for q in QUADS if R.case(q)["x"].shape[1] > 12000):
        c = R.case(name)
        n = c["x"].shape[1]
        assert n in (R.N3, R.N3 - 1)
        x = c["x"].copy()
        x[:, 8000:] = R.noise(x.shape[0], n - 8000, 55) * F32(3)
        a, b = run(c), run(c, x)
        assert same_bits(a[:, :8000], b[:, :8000]), name
        assert not same_bits(a[:, 8000:], b[:, 8000:]), name


def test_a_nan_cutoff_poisons_what_follows_and_nothing_before():
    got, clean = run(R.case("nan_low3")), run(R.case("clean_low3"))
    f = R.POISON_FRAME
    assert same_bits(got[:, :f], clean[:, :f])
    assert np.all(np.isnan(got[:, f:]))


def test_a_damping_above_1_poisons_an_odd_order_from_that_frame_on():
    got, clean = run(R.case("over1_highshelf3")), run(R.case("clean_highshelf3"))
    f = R.POISON_FRAME
    assert same_bits(got[:, :f], clean[:, :f])
    assert np.all(np.isnan(got[:, f:]))


def test_order_zero():
    """a copy; silence for the notch; the copy times amp( gain / 2 ) for the 1-pole shelves"""
    for c in R.CASES:
        if c["order"] != 0:
            continue
        want = R.expected(c["name"], F32)
        if c["kind"] == R.NOTCH:
            assert not np.any(want)
        elif c["kind"] > R.SHELF1_HIGH:
            assert same_bits(want, c["x"])
        else:
            assert same_bits(want, c["x"] * R.amp(np.broadcast_to(np.asarray(c["gain"], F32), (c["x"].shape[1],)) / F32(2)))
        assert same_bits(run(c), want) and same_bits(run_dev(c), want), c["name"]
        if c["kind"] != R.NOTCH:
            assert same_bits(run_dev(c, alias=True), want), c["name"]
    assert {c["kind"] for c in R.CASES if c["order"] == 0} == set(range(9))
