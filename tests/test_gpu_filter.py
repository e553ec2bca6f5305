"""Audio::filter_1pole_lowpass / _highpass / _repeat_low / _repeat_high on the MI355X (flan_amd/csrc/filter.hip) against the NumPy
restatement (tests/filter_reference.py): the fp32 loop and the fp64 truth.  Errors are divided by the rms and the peak of the INPUT.
Bounds: DESIGN.md 4.15 lists the measured values they are set from (<= 30 % above)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import filter_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
# against the fp32 restatement, over all cases that do not stall: rms( got - want ) / rms( x ) and max | got - want | / max | x |.
# The device against the restatement, never the device against itself
REL_RMS_BOUND = 1.2e-7          # measured on the MI355X at most 9.538e-8 (rhigh16_noise_sweep)
REL_MAX_BOUND = 6.0e-7          # measured on the MI355X at most 4.768e-7 (low8_noise_sweep): 4 fp32 ulps of the input's peak
# against the fp64 truth: at most 4 x the restatement's own error on the same case, or 8 fp32 ulps of the input's scale where that is smaller
TRUTH_FACTOR = 4.0
TRUTH_FLOOR = 8 * 2.0 ** -23
# the cases whose length is a multiple of 4, over one block and over three, 2 and 3 channels: there (and only there) the kernels read and
# write 16 bytes at a time, so every property below is held on them as well
QUADS = tuple(c["name"] for c in R.CASES if c["parity"] and c["x"].shape[1] % 4 == 0 and c["x"].shape[1] >= R.BLOCK)
assert len(QUADS) == 8


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def run(c, x=None):
    return fa.filter_1pole(c["x"] if x is None else x, c["sr"], c["cutoff"], kind=c["kind"], order=c["order"])


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
    d_ws = torch.full((fa.filter_1pole_workspace_bytes(ch, n),), 0xFF, dtype=torch.uint8, device=dev)
    cutoff = c["cutoff"] if np.isscalar(c["cutoff"]) else to_dev(c["cutoff"])
    fa.filter_1pole_dev(d_x, ch, n, c["sr"], cutoff, c["kind"], c["order"], d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("name", R.PARITY_IDS)
def test_against_the_restatement_and_the_truth(name):
    c = R.case(name)
    got = run(c)
    want, truth = R.expected(name, F32), R.expected(name, F64)
    assert got.shape == want.shape and got.dtype == F32
    rel_rms, rel_max = R.errors(got, want, c["x"])
    t_rms, t_max = R.errors(got, truth, c["x"])
    own_rms, own_max = R.errors(want, truth, c["x"])
    differ = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    print("%s%s: vs restatement rel_rms=%.3e rel_max=%.3e (%d of %d differ); vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
          % (name, " (stalls)" if R.stalls(name) else "", rel_rms, rel_max, differ, got.size, t_rms, t_max, own_rms, own_max))
    failures = []
    if not R.stalls(name) and not (rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND):
        failures.append(("restatement", rel_rms, rel_max))
    if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
        failures.append(("truth", t_rms, t_max, own_rms, own_max))
    assert not failures, failures


def test_host_and_device_forms_are_bit_identical():
    for name in ("low8_noise_sweep", "high3_noise_sweep", "rlow16_noise_wobble", "high4_noise_wobble", "n1_low3_noise_sweep", "n4095_low8_noise_sweep") + QUADS:
        c = R.case(name)
        assert same_bits(run(c), run_dev(c)), name


def test_out_may_alias_the_input():
    for name in ("low8_noise_sweep", "high1_sine_random", "n1023_low2_noise_wobble", "rhigh16_noise_sweep", "low4_noise_1k") + QUADS:
        c = R.case(name)
        assert same_bits(run_dev(c), run_dev(c, alias=True)), name


def test_two_runs_are_bit_identical():
    for name in ("high8_sine_random", "low3_sine_random"):
        assert same_bits(run(R.case(name)), run(R.case(name))), name


def test_a_channel_does_not_depend_on_the_channels_filtered_with_it():
    for name in ("low8_noise_sweep", "high2_noise_1k") + QUADS:
        c = R.case(name)
        out = run(c)
        for k in range(c["x"].shape[0]):
            assert same_bits(run(c, c["x"][k:k + 1])[0], out[k]), (name, k)


@pytest.mark.parametrize("frames", [1, 7, 64])
def test_the_run_length_changes_nothing_beyond_rounding(frames):
    """7: runs that do not start on 16-byte boundaries (the scalar loads); 1: 49 blocks a channel for 12 305 frames; 64: one, and with
    the lengths that are multiples of 4 the 16-byte loads over runs of 16 quads"""
    for name in ("low8_noise_sweep", "high3_noise_sweep", "rhigh16_noise_sweep") + QUADS:
        c = R.case(name)
        assert not R.stalls(name)
        out = run(c)
        with fa.filter_run_forced(frames):
            out_f = run(c)
        for what, want in (("the default run", out), ("the restatement", R.expected(name, F32))):
            rel_rms, rel_max = R.errors(out_f, want, c["x"])
            print("%s run %d vs %s: rel_rms=%.3e rel_max=%.3e" % (name, frames, what, rel_rms, rel_max))
            assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (name, what)


def test_later_input_does_not_reach_earlier_output():
    """a carry taken from an inclusive total would"""
    for name in ("low8_noise_sweep", "high3_noise_sweep") + tuple(q for q in QUADS if R.case(q)["x"].shape[1] > 12000):
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
    f = R.NAN_FRAME
    assert same_bits(got[:, :f], clean[:, :f])
    assert np.all(np.isnan(got[:, f:]))


def test_order_zero_copies_and_no_repeats_are_silence():
    for name in ("low0_noise_1k", "high0_noise_wobble"):
        c = R.case(name)
        assert same_bits(run(c), c["x"]) and same_bits(run_dev(c), c["x"]) and same_bits(run_dev(c, alias=True), c["x"]), name
    for name in ("rlow0_noise_1k", "rhigh0_sine_random"):
        c = R.case(name)
        zeros = np.zeros_like(c["x"])
        assert same_bits(run(c), zeros) and same_bits(run_dev(c), zeros) and same_bits(run_dev(c, alias=True), zeros), name


def test_the_nyquist_case_stays_finite():
    got = run(R.case("nyquist_low3"))
    assert np.all(np.isfinite(got[np.isfinite(R.expected("nyquist_low3"))]))


# ---- rows longer than one pass of the carry kernel ---------------------------------------------------------------
# k_scan_carry turns 256 block totals a pass into carried states; every case above is 49 blocks at the most.  The rows of
# filter_reference.LONG are 256 blocks exactly, 257, and 516 in three passes at a run of 1, and 258 at the default run.
THREE_PASSES = ("low3_n%d_run1" % R.N_THREE_PASSES, "high2_n%d_run1" % R.N_THREE_PASSES)


def run_long(c, x=None):
    with fa.filter_run_forced(c["run"] or 0):
        return run(c, x)


def run_long_dev(c, alias=False):
    with fa.filter_run_forced(c["run"] or 0):              # the workspace is sized for the run as well
        return run_dev(dict(c, x=np.array(c["x"]), cutoff=np.array(c["cutoff"])), alias)      # copies: the long cases are read-only


@pytest.mark.parametrize("name", R.LONG_IDS)
def test_rows_longer_than_one_pass_of_the_carry_kernel(name):
    """the conditions of test_against_the_restatement_and_the_truth over the whole row, over every pass's frames and over the first
    block of every pass after the first, each divided by the rms and the peak of the whole input"""
    c = R.long_case(name)
    got = run_long(c)
    want, truth = R.long_expected(name, F32), R.long_expected(name, F64)
    assert got.shape == want.shape and got.dtype == F32
    failures = []
    for label, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max) in R.figures(got, want, truth, c["x"], c["run"] or R.RUN):
        print("%s %s: vs restatement rel_rms=%.3e rel_max=%.3e; vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
              % (name, label, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
        if not (rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND):
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
    """a 1 Hz first-order low-pass forgets 1.9e-4 of its state over a pass: what frames [0, 256) hold moves the output at frames
    65 536 and 131 072, by 3e5 and by 60 ulps in the scan model (tests/test_filter_reference.py)"""
    x, other = R.memory_inputs()
    with fa.filter_run_forced(1):
        a = fa.filter_1pole(x, R.SR, R.MEMORY_CUTOFF, kind=R.BUTTERWORTH_LOW, order=1)
        b = fa.filter_1pole(other, R.SR, R.MEMORY_CUTOFF, kind=R.BUTTERWORTH_LOW, order=1)
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
    c = R.long_case(THREE_PASSES[0])
    host = run_long(c)
    assert same_bits(run_long_dev(c), host)
    assert same_bits(run_long_dev(c, alias=True), host)           # out aliasing the input
    assert same_bits(run_long(c), host)                           # a second call
