"""Audio::compress, modify_volume and set_volume on the MI355X (flan_amd/csrc/compress.hip) against the NumPy restatement
(tests/compress_reference.py): the fp32 loop and the fp64 truth.  Bounds: DESIGN.md 4.14 lists the measured values they are set from
(<= 30 % above).  Every figure is printed before it is held."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import compress_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
# against the fp32 restatement, over all cases: relative rms error, and max abs error / max |ref|, of the output and of the gain curve
REL_RMS_BOUND = 9.8e-7          # measured at most 7.553e-7 (per_frame, the gain curve)
REL_MAX_BOUND = 1.05e-6         # measured at most 8.139e-7 (attack0, the output)
# the dc case alone: there the sequential fp32 loop stalls short of the level it approaches (a y + ( 1 - a ) x stops moving once the step
# is under half an ulp of y) and is itself 1.413e-5 / 8.657e-6 from the fp64 truth; every run of the scan starts from the fp64 state, so
# the device follows the truth (9.0e-7 / 1.2e-6 from it) and is that far from the restatement
DC_REL_RMS_BOUND = 1.8e-5       # measured 1.389e-5
DC_REL_MAX_BOUND = 1.1e-5       # measured 8.651e-6
# against the fp64 truth: at most 4 x the restatement's own error on the same case, or 8 fp32 ulps of the peak where that is smaller
TRUTH_FACTOR = 4.0
TRUTH_FLOOR = 8 * 2.0 ** -23


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def run(c):
    return fa.compress(c["x"], c["sr"], sidechain=c["side"], want_gain=True, **c["params"])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def to_dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, F32)).to(torch.device("cuda", 0))


def run_dev(c, alias=False):
    """the _dev form with its workspace filled with 0xFF and its outputs with NaN beforehand"""
    dev = torch.device("cuda", 0)
    ch, n = c["x"].shape
    side = c["x"] if c["side"] is None else c["side"]
    d_x, d_side = to_dev(c["x"]), to_dev(side)
    d_out = d_x if alias else torch.full((ch, n), float("nan"), dtype=torch.float32, device=dev)
    d_gain = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    d_ws = torch.full((fa.compress_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=dev)
    params = {k: (v if np.isscalar(v) else to_dev(v)) for k, v in c["params"].items()}
    fa.compress_dev(d_x, ch, n, c["sr"], d_x if c["side"] is None else d_side, side.shape[0], side.shape[1], d_out, d_gain, d_ws, **params)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_gain.cpu().numpy()


@pytest.mark.parametrize("name", R.IDS)
def test_against_the_restatement_and_the_truth(name):
    c = R.case(name)
    out, gain = run(c)
    want_out, want_gain = R.expected(name, F32)
    true_out, true_gain = R.expected(name, F64)
    assert out.shape == want_out.shape and gain.shape == want_gain.shape
    failures = []
    for what, got, want, truth in (("out", out, want_out, true_out), ("gain", gain, want_gain, true_gain)):
        rel_rms, rel_max = R.errors(got, want)
        t_rms, t_max = R.errors(got, truth)
        own_rms, own_max = R.errors(want, truth)
        differ = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
        print("%s %s: vs restatement rel_rms=%.3e rel_max=%.3e (%d of %d differ); vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
              % (name, what, rel_rms, rel_max, differ, got.size, t_rms, t_max, own_rms, own_max))
        rms_bound, max_bound = (DC_REL_RMS_BOUND, DC_REL_MAX_BOUND) if name == "dc" else (REL_RMS_BOUND, REL_MAX_BOUND)
        if not (rel_rms <= rms_bound and rel_max <= max_bound):
            failures.append((what, "restatement", rel_rms, rel_max))
        if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
            failures.append((what, "truth", t_rms, t_max, own_rms, own_max))
    assert not failures, failures


def test_ratio_one_and_all_negative_input_come_back_bit_identical():
    for name in ("ratio1", "negative"):
        out, gain = run(R.case(name))
        assert same_bits(out, R.case(name)["x"]), name
        assert np.all(gain == 1.0), name


def test_host_and_device_forms_are_bit_identical():
    for name in ("bursts_n%d" % (R.BLOCK + 1), "per_frame", "side_mono", "side_longer", "bursts_n1"):
        c = R.case(name)
        out, gain = run(c)
        d_out, d_gain = run_dev(c)
        assert same_bits(out, d_out) and same_bits(gain, d_gain), name


def test_two_runs_are_bit_identical():
    for name in ("per_frame_knee6_3blocks", "knee6"):
        a, b = run(R.case(name)), run(R.case(name))
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])


def test_out_may_alias_the_audio():
    for name in ("per_frame", "side_mono", "bursts_n%d" % (R.WAVE - 1)):
        c = R.case(name)
        separate, aliased = run_dev(c), run_dev(c, alias=True)
        assert same_bits(separate[0], aliased[0]) and same_bits(separate[1], aliased[1]), name


@pytest.mark.parametrize("frames", [1, 7, 64])
def test_the_run_length_changes_nothing_beyond_rounding(frames):
    """7: runs that do not start on 16-byte boundaries (the scalar loads); 1: 48 blocks of the scan for 12 305 frames; 64: one"""
    for name in ("per_frame_knee6_3blocks", "bursts_n%d" % (R.BLOCK - 1)):
        c = R.case(name)
        out, gain = run(c)
        with fa.compress_run_forced(frames):
            out_f, gain_f = run(c)
        for got, want in ((out_f, out), (gain_f, gain)):
            rel_rms, rel_max = R.errors(got, want)
            print("%s run %d: rel_rms=%.3e rel_max=%.3e" % (name, frames, rel_rms, rel_max))
            assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND
        want_out, want_gain = R.expected(name, F32)
        for got, want in ((out_f, want_out), (gain_f, want_gain)):
            rel_rms, rel_max = R.errors(got, want)
            assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND


def test_the_gain_does_not_depend_on_the_channel_count():
    c = R.case("side_mono")                                               # three channels against a fixed mono sidechain
    out, gain = run(c)
    for k in range(3):
        mono, mono_gain = fa.compress(c["x"][k:k + 1], c["sr"], sidechain=c["side"], want_gain=True, **c["params"])
        assert same_bits(mono[0], out[k]) and same_bits(mono_gain, gain), k


@pytest.mark.parametrize("ch,n", [(1, 1), (3, 1001), (2, 4096), (3, 4098)])
def test_audio_gain_dev_is_numpys_product(ch, n):
    rng = np.random.default_rng(n)
    x = rng.uniform(-1, 1, (ch, n)).astype(F32)
    curve = rng.uniform(-2, 2, n).astype(F32)
    d_x = to_dev(x)
    d_out = torch.full((ch, n), float("nan"), dtype=torch.float32, device=d_x.device)
    fa.audio_gain_dev(d_x, ch, n, to_dev(curve), d_out)
    assert same_bits(d_out.cpu().numpy(), x * curve[None, :])
    fa.audio_gain_dev(d_x, ch, n, 0.3, d_out)
    assert same_bits(d_out.cpu().numpy(), x * F32(0.3))
    fa.audio_gain_dev(d_x, ch, n, to_dev(curve), d_x)                     # in place
    assert same_bits(d_x.cpu().numpy(), x * curve[None, :])
    assert same_bits(d_out.cpu().numpy(), R.modify_volume(x, 0.3))


def set_volume_dev(x, sr, level):
    ch, n = x.shape
    d_x = to_dev(x)
    d_out = torch.full((ch, n), float("nan"), dtype=torch.float32, device=d_x.device)
    d_ws = torch.full((fa.audio_set_volume_workspace_bytes(ch, n),), 0xFF, dtype=torch.uint8, device=d_x.device)
    fa.audio_set_volume_dev(d_x, ch, n, sr, level if np.isscalar(level) else to_dev(level), d_out, d_ws)
    return d_out.cpu().numpy()


@pytest.mark.parametrize("ch,n", [(1, 2), (3, 1001), (2, 4096), (2, 300001)])
def test_audio_set_volume_dev_is_the_restatement(ch, n):
    rng = np.random.default_rng(n)
    x = (0.7 * rng.uniform(-1, 1, (ch, n))).astype(F32)
    level = rng.uniform(0.1, 1.0, n).astype(F32)
    assert same_bits(set_volume_dev(x, 48000.0, 0.9), R.set_volume(x, 48000.0, 0.9))
    assert same_bits(set_volume_dev(x, 44100.0, level), R.set_volume(x, 44100.0, level))


def test_audio_set_volume_dev_edge_cases():
    zeros = np.zeros((2, 1000), F32)
    assert same_bits(set_volume_dev(zeros, 48000.0, 0.9), zeros)
    one = np.full((2, 1), 0.3, F32)                                       # one frame: nothing is looked at, the maximum is 0
    assert same_bits(set_volume_dev(one, 48000.0, 0.9), one)
    rng = np.random.default_rng(3)
    x = (0.25 * rng.uniform(-1, 1, (2, 1000))).astype(F32)
    x[1, 500] = -0.5
    x[0, -1] = 0.9                                                        # the peak sits in the last frame, which is not looked at
    y = set_volume_dev(x, 48000.0, 0.8)
    assert same_bits(y, x * (F32(0.8) / F32(0.5)))
    assert same_bits(y, R.set_volume(x, 48000.0, 0.8))


# ---- rows longer than one pass of the carry kernel ---------------------------------------------------------------
# k_scan_carry turns 256 block totals a pass into carried states; every case above is 49 blocks at the most.  The rows of
# compress_reference.LONG are 256 blocks exactly, 257, and 516 in three passes at a run of 1, and 258 at the default run.
THREE_PASSES = "bursts_n%d_run1" % R.N_THREE_PASSES
# Against the fp32 restatement these rows have bounds of their own.  The fp32 loop itself is further from the truth here than on the
# short cases (1.4e-6 rms over the third pass of bursts_n131857_run1, 2.6e-6 at the most over bursts_n1052688: the last quarter's attack
# of 50 ms is 2400 frames of accumulation), the device starts every run from the fp64 state and is nearer the truth than the loop over
# every whole row, so its distance from the loop is the loop's own error: measured on the MI355X at most 1.127e-6 (bursts_n131857_run1, the gain
# curve over pass 2) and 2.325e-6 (bursts_n1052688, the gain curve, whole).  REL_RMS_BOUND and REL_MAX_BOUND stay as they are
LONG_REL_RMS_BOUND = 1.45e-6
LONG_REL_MAX_BOUND = 3.0e-6


def run_long(c, x=None):
    with fa.compress_run_forced(c["run"] or 0):
        return run(c if x is None else dict(c, x=x))


def run_long_dev(c, alias=False):
    with fa.compress_run_forced(c["run"] or 0):            # the workspace is sized for the run as well
        params = {k: v if np.isscalar(v) else np.array(v) for k, v in c["params"].items()}         # copies: the long cases are read-only
        return run_dev(dict(c, x=np.array(c["x"]), params=params), alias)


@pytest.mark.parametrize("name", R.LONG_IDS)
def test_rows_longer_than_one_pass_of_the_carry_kernel(name):
    """the conditions of test_against_the_restatement_and_the_truth on the output and on the gain curve, over the whole row, over every
    pass's frames and over the first block of every pass after the first, each divided by the rms and the peak of the whole reference.
    Against the restatement: LONG_REL_RMS_BOUND / LONG_REL_MAX_BOUND"""
    c = R.long_case(name)
    out, gain = run_long(c)
    want_out, want_gain = R.long_expected(name, F32)
    true_out, true_gain = R.long_expected(name, F64)
    assert out.shape == want_out.shape and gain.shape == want_gain.shape
    failures = []
    for what, got, want, truth in (("out", out, want_out, true_out), ("gain", gain, want_gain, true_gain)):
        for label, (rel_rms, rel_max), (t_rms, t_max), (own_rms, own_max) in R.figures(got, want, truth, c["run"] or R.RUN):
            print("%s %s %s: vs restatement rel_rms=%.3e rel_max=%.3e; vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
                  % (name, what, label, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
            if not (rel_rms <= LONG_REL_RMS_BOUND and rel_max <= LONG_REL_MAX_BOUND):
                failures.append((what, label, "restatement", rel_rms, rel_max))
            if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
                failures.append((what, label, "truth", t_rms, t_max, own_rms, own_max))
    assert not failures, failures


def test_later_input_does_not_reach_an_earlier_pass_of_the_carry_kernel():
    cut = R.PASS_RUNS
    c = R.long_case(THREE_PASSES)
    x = c["x"].copy()
    x[:, cut:] = R.bursts(x.shape[0], x.shape[1] - cut, 56) * F32(0.7)
    (a_out, a_gain), (b_out, b_gain) = run_long(c), run_long(c, x)
    assert same_bits(a_out[:, :cut], b_out[:, :cut]) and same_bits(a_gain[:cut], b_gain[:cut])
    assert not same_bits(a_gain[cut:cut + 256], b_gain[cut:cut + 256]) and not same_bits(a_gain[2 * cut:], b_gain[2 * cut:])


def test_long_rows_host_and_device_forms_are_bit_identical():
    c = R.long_case(THREE_PASSES)
    host = run_long(c)
    for other in (run_long_dev(c), run_long_dev(c, alias=True), run_long(c)):       # the _dev form, out aliasing the audio, a second call
        assert same_bits(other[0], host[0]) and same_bits(other[1], host[1])
