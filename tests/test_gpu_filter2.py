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


# ---- rows longer than one pass of the carry kernel ---------------------------------------------------------------
# k_scan_carry turns 256 block totals a pass into carried states; every case above is 49 blocks at the most.  The rows of
# filter2_reference.LONG are 256 blocks exactly, 257, and 516 in three passes at a run of 1, and 258 at the default run.
THREE_PASSES = ("low2_d025_n%d_run1" % R.N_THREE_PASSES, "highshelf3_dcurve_p6_n%d_run1" % R.N_THREE_PASSES)


def run_long(c, x=None):
    with fa.filter_run_forced(c["run"] or 0):
        return run(c, x)


def run_long_dev(c, alias=False):
    with fa.filter_run_forced(c["run"] or 0):              # the workspace is sized for the run as well
        copies = {k: v if np.isscalar(v) else np.array(v) for k, v in c.items() if k in ("x", "cutoff", "damping", "gain")}      # the long cases are read-only
        return run_dev(dict(c, **copies), alias)


@pytest.mark.parametrize("name", R.LONG_IDS)
def test_rows_longer_than_one_pass_of_the_carry_kernel(name):
    """the conditions of test_against_the_restatement_and_the_truth (parity cases) over the whole row, over every pass's frames and over
    the first block of every pass after the first, each divided by the rms and the peak of the whole input"""
    c = R.long_case(name)
    got = run_long(c)
    want, truth = R.long_expected(name, F32), R.long_expected(name, F64)
    assert got.shape == want.shape and got.dtype == F32
    failures = []
    run_ = c["run"] or R.RUN
    for (label, lo, hi), (_, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max)) in zip(R.windows(got.shape[1], run_), R.figures(got, want, truth, c["x"], run_)):
        print("%s %s: vs restatement rel_rms=%.3e rel_max=%.3e; vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
              % (name, label, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
        if not (rel_rms <= R.rms_bound(lo, hi) and rel_max <= REL_MAX_BOUND):       # a window of one frame: filter2_reference.rms_bound
            failures.append((label, "restatement", rel_rms, rel_max))
        if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
            failures.append((label, "truth", t_rms, t_max, own_rms, own_max))
    assert not failures, failures


def test_later_input_does_not_reach_an_earlier_pass_of_the_carry_kernel():
    cut = R.PASS_RUNS
    for name in THREE_PASSES:
        c = R.long_case(name)
        x = c["x"].copy()
        x[:, cut:] = R.noise(x.shape[0], x.shape[1] - cut, 56) * F32(3)
        a, b = run_long(c), run_long(c, x)
        assert same_bits(a[:, :cut], b[:, :cut]), name
        assert not np.any(a[:, cut] == b[:, cut]) and not same_bits(a[:, 2 * cut:], b[:, 2 * cut:]), name


def test_the_state_flows_through_a_whole_pass_of_the_carry_kernel():
    """under the swept cutoff the damping 0.25 low-pass has forgotten frames [0, 256) long before frame 65 536
    (tests/test_filter2_reference.py), so the matrix of a pass's total is held on a 1 Hz low-pass of damping 1, two equal real poles:
    what frames [0, 256) hold moves the output at frames 65 536 and 131 072"""
    x, other = R.memory_inputs()
    with fa.filter_run_forced(1):
        a = fa.filter2(x, R.SR, R.MEMORY_CUTOFF, 1.0, 0.0, kind=R.LOW, order=1)
        b = fa.filter2(other, R.SR, R.MEMORY_CUTOFF, 1.0, 0.0, kind=R.LOW, order=1)
    for frame in (R.PASS_RUNS, 2 * R.PASS_RUNS):
        assert not np.any(a[:, frame] == b[:, frame]), frame


def test_long_rows_are_independent():
    """k_scan_carry finds its row's totals at blockIdx.x * blocks, with 516 blocks a row"""
    for name in THREE_PASSES:
        c = R.long_case(name)
        assert c["x"].shape[0] == 3
        out = run_long(c)
        for k in range(3):
            assert same_bits(run_long(c, c["x"][k:k + 1])[0], out[k]), (name, k)
        assert same_bits(run_long(c, c["x"][::-1])[::-1], out), name


def test_long_rows_host_and_device_forms_are_bit_identical():
    for name in THREE_PASSES:
        c = R.long_case(name)
        host = run_long(c)
        assert same_bits(run_long_dev(c), host), name
        assert same_bits(run_long_dev(c, alias=True), host), name    # out aliasing the input
        assert same_bits(run_long(c), host), name                    # a second call
