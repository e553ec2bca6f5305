"""hilbert_phase_diff_network, Audio::halfband_modulate, Audio::shift_frequency and Audio::halfband_multiply on the MI355X
(flan_amd/csrc/halfband.hip) against the NumPy restatement (tests/halfband_reference.py): the fp32 loop and the fp64 truth.  Errors are
divided by the rms and the peak of the INPUT (multiply: the products of the operands').  The bounds (halfband_reference.BOUNDS, a pair per
kind of input) are twice the worst the MI355X measured over the cases: DESIGN.md 4.17."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import filter_reference as R1
import halfband_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
BOUNDS, TRUTH_FACTOR, TRUTH_FLOOR = R.BOUNDS, R.TRUTH_FACTOR, R.TRUTH_FLOOR
BIG, QUADS, RAGGED = "n9001_c3_noise_48_run0", "n8192_c3_noise_48_run0", "n1000_c3_noise_48_run1"


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def to_dev(v):
    return torch.from_numpy(np.ascontiguousarray(v, F32)).to(torch.device("cuda", 0))


def run(c, x=None, run_length=None):
    """the five results of a case through the host forms, at the case's run length"""
    x = c["x"] if x is None else x
    with fa.halfband_run_forced(c["run"] if run_length is None else run_length):
        first, second = fa.hilbert(x, c["sr"])
        return {"first": first, "second": second, "rows": fa.halfband_modulate(x, c["sr"], c["re"], c["im"]),
                "phase": fa.halfband_modulate(x, c["sr"], phase=c["phase"]), "multiply": fa.halfband_multiply(x, c["sr"], c["b"], c["b_sr"])}


def run_dev(c, alias=False):
    """the same through the _dev forms, every workspace filled with 0xFF and every output with NaN beforehand; alias: every output that has
    the input's shape is the input's own buffer (a fresh copy of it per call)"""
    dev = torch.device("cuda", 0)
    ch, n = c["x"].shape
    o_ch, o_n = min(ch, c["b"].shape[0]), min(n, c["b"].shape[1])

    def ws(w_ch, w_n):
        return torch.full((fa.halfband_workspace_bytes(w_ch, w_n),), 0xFF, dtype=torch.uint8, device=dev)

    def fresh(shape=(ch, n)):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    out = {}
    with fa.halfband_run_forced(c["run"]):
        d_x, d_second = to_dev(c["x"]), fresh()
        d_first = d_x if alias else fresh()
        fa.hilbert_dev(d_x, ch, n, c["sr"], d_first, d_second, ws(ch, n))
        out["first"], out["second"] = d_first.cpu().numpy(), d_second.cpu().numpy()
        d_x, d_first = to_dev(c["x"]), fresh()
        d_second = d_x if alias else fresh()
        fa.hilbert_dev(d_x, ch, n, c["sr"], d_first, d_second, ws(ch, n))
        assert same_bits(out["first"], d_first.cpu().numpy())
        out["second"] = d_second.cpu().numpy()
        d_x = to_dev(c["x"])
        d_out = d_x if alias else fresh()
        fa.halfband_modulate_dev(d_x, ch, n, c["sr"], to_dev(c["re"]), to_dev(c["im"]), None, d_out, ws(ch, n))
        out["rows"] = d_out.cpu().numpy()
        d_x = to_dev(c["x"])
        d_out = d_x if alias else fresh()
        fa.halfband_modulate_dev(d_x, ch, n, c["sr"], 0.0, 0.0, to_dev(c["phase"]), d_out, ws(ch, n))
        out["phase"] = d_out.cpu().numpy()
        d_x, d_b, d_out = to_dev(c["x"]), to_dev(c["b"]), fresh((o_ch, o_n))
        fa.halfband_multiply_dev(d_x, ch, n, c["sr"], d_b, c["b"].shape[0], c["b"].shape[1], c["b_sr"], d_out, ws(o_ch, o_n))
        out["multiply"] = d_out.cpu().numpy()
    torch.cuda.synchronize()
    return out


def held(name, got, what=""):
    """the two criteria for the five results of a case: [] or what failed"""
    c = R.case(name)
    want, truth, scales = R.expected(name, F32), R.expected(name, F64), R.scales(c)
    rel_rms_bound, rel_max_bound = BOUNDS[c["kind"]]
    failures = []
    for r in R.RESULTS:
        assert got[r].shape == want[r].shape and got[r].dtype == F32, (name, r)
        rel_rms, rel_max = R.errors(got[r], want[r], *scales[r])
        t_rms, t_max = R.errors(got[r], truth[r], *scales[r])
        own_rms, own_max = R.errors(want[r], truth[r], *scales[r])
        print("%s %s%s: vs restatement rel_rms=%.3e rel_max=%.3e; vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
              % (name, r, what, rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
        if not (rel_rms <= rel_rms_bound and rel_max <= rel_max_bound):
            failures.append((r, "restatement", rel_rms, rel_max))
        if not (t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)):
            failures.append((r, "truth", t_rms, t_max, own_rms, own_max))
    return failures


@pytest.mark.parametrize("name", R.IDS)
def test_against_the_restatement_and_the_truth(name):
    failures = held(name, run(R.case(name)))
    assert not failures, failures


def test_host_and_device_forms_are_bit_identical():
    for name in (BIG, QUADS, RAGGED, "n1_c1_noise_48_run1", "n256_c1_step_44_run1", "n8192_c3_impulse_44_run0"):
        host, dev = run(R.case(name)), run_dev(R.case(name))
        for r in R.RESULTS:
            assert same_bits(host[r], dev[r]), (name, r)


def test_two_runs_are_bit_identical():
    for name in (BIG, QUADS, RAGGED):
        a, b = run(R.case(name)), run(R.case(name))
        for r in R.RESULTS:
            assert same_bits(a[r], b[r]), (name, r)


def test_a_channel_does_not_depend_on_the_channels_beside_it():
    for name in (BIG, QUADS, RAGGED, "n255_c3_noise_48_run1"):
        c = R.case(name)
        out = run(c)
        assert c["x"].shape[0] == 3
        for k in range(3):
            alone = run(c, c["x"][k:k + 1])
            for r in ("first", "second", "rows", "phase"):
                assert same_bits(alone[r][0], out[r][k]), (name, r, k)
        # multiply pairs channel k with the second operand's channel k
        assert same_bits(run(c, c["x"][:1])["multiply"][0], out["multiply"][0]), name


@pytest.mark.parametrize("frames", [1, 4, 16, 64])
def test_the_run_length_changes_nothing_beyond_rounding(frames):
    """1: 36 blocks a channel for 9001 frames; 4: the shortest run of whole quads; 64: one block"""
    for name in (BIG, QUADS):
        failures = held(name, run(R.case(name), run_length=frames), " run %d" % frames)
        assert not failures, failures


def test_more_than_1024_blocks_a_channel():
    """k_hb_carry takes 1024 block totals a pass: at run 1, 262 444 frames are 1026 blocks, a second pass from the state the first left.  The
    sequential restatement would take a quarter of a minute here; the default run (65 blocks, one pass), held to the restatement by the
    cases, stands in for it, within the same bounds"""
    n, sr = 1024 * 256 + 300, 48000.0
    x, phase = R.noise(1, n, 77), R.phase_row(n, sr)
    rms, peak = R.scale(x)
    with fa.halfband_run_forced(1):
        assert fa.halfband_workspace_bytes(1, n) == 26400 + 640 * 1026
        one = fa.hilbert(x, sr) + (fa.halfband_modulate(x, sr, phase=phase),)
    default = fa.hilbert(x, sr) + (fa.halfband_modulate(x, sr, phase=phase),)
    for what, a, b in zip(("first", "second", "phase"), one, default):
        rel_rms, rel_max = R.errors(a, b, rms, peak)
        tail_rms, tail_max = R.errors(a[:, 1024 * 256:], b[:, 1024 * 256:], rms, peak)
        print("1026 blocks, %s: run 1 vs the default run rel_rms=%.3e rel_max=%.3e; the second pass's frames %.3e %.3e" % (what, rel_rms, rel_max, tail_rms, tail_max))
        assert rel_rms <= BOUNDS["noise"][0] and rel_max <= BOUNDS["noise"][1], what
        assert tail_rms <= BOUNDS["noise"][0] and tail_max <= BOUNDS["noise"][1], what


def test_later_input_does_not_reach_earlier_output():
    """a carry taken from an inclusive total would"""
    for name in (BIG, QUADS, RAGGED):
        c = R.case(name)
        n = c["x"].shape[1]
        cut = 2 * n // 3
        x = c["x"].copy()
        x[:, cut:] = R.noise(x.shape[0], n - cut, 55) * F32(3)
        a, b = run(c), run(c, x)
        for r in R.RESULTS:
            assert same_bits(a[r][:, :cut], b[r][:, :cut]), (name, r)
            assert not same_bits(a[r][:, cut:], b[r][:, cut:]), (name, r)


def test_an_output_may_be_the_input():
    for name in (BIG, QUADS, RAGGED, "n3_c3_impulse_44_run1"):
        plain, aliased = run_dev(R.case(name)), run_dev(R.case(name), alias=True)
        for r in R.RESULTS:
            assert same_bits(plain[r], aliased[r]), (name, r)


def test_a_nan_sample_poisons_what_follows_and_nothing_before():
    for name, frame in ((BIG, 5000), (QUADS, 4100), (RAGGED, 300)):
        c = R.case(name)
        x = c["x"].copy()
        x[1, frame] = np.nan
        clean, got = run(c), run(c, x)
        for r in R.RESULTS:
            rows = range(got[r].shape[0])
            for k in rows:
                if k == 1:
                    assert same_bits(got[r][k, :frame], clean[r][k, :frame]), (name, r)
                    assert np.all(np.isnan(got[r][k, frame:])), (name, r)
                else:
                    assert same_bits(got[r][k], clean[r][k]), (name, r, k)


# ---- Audio::shift_frequency, as flan_amd/host/Audio.cpp runs it: the two filter calls, then the modulation with the host-made phase ----
def shift_frequency(x, sr, shift):
    lp, hp, phase = R.shift_curves(shift, sr)
    y = fa.filter_1pole(x, sr, lp, kind=fa.FILTER_BUTTERWORTH_LOW, order=8)
    y = fa.filter_1pole(y, sr, hp, kind=fa.FILTER_BUTTERWORTH_HIGH, order=8)
    return fa.halfband_modulate(y, sr, phase=phase)


def test_shift_frequency_with_a_shift_that_changes_sign():
    n, sr = 9001, 48000.0
    x = R.noise(2, n, 31)
    shift = (300.0 * np.sin(2 * np.pi * 4.0 * np.arange(n) / sr + 1.0)).astype(F32)
    assert shift.min() < -200 and shift.max() > 200
    got = shift_frequency(x, sr, shift)
    want, truth = R.shift_frequency(x, sr, shift, dtype=F32), R.shift_frequency(x, sr, shift, dtype=F64)
    rms, peak = R.scale(x)
    rel_rms, rel_max = R.errors(got, want, rms, peak)
    t_rms, t_max = R.errors(got, truth, rms, peak)
    own_rms, own_max = R.errors(want, truth, rms, peak)
    print("shift_frequency: vs restatement rel_rms=%.3e rel_max=%.3e; vs truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)"
          % (rel_rms, rel_max, t_rms, t_max, own_rms, own_max))
    assert rel_rms <= R.SHIFT_BOUNDS[0] and rel_max <= R.SHIFT_BOUNDS[1]
    assert t_rms <= max(TRUTH_FACTOR * own_rms, TRUTH_FLOOR) and t_max <= max(TRUTH_FACTOR * own_max, TRUTH_FLOOR)


def rejection_db(y, sr):
    """the power at 1250 Hz over the power at 750 Hz in the second half of y [n], Hann windowed, in dB"""
    half = y[len(y) // 2:].astype(F64)
    spec = np.abs(np.fft.rfft(half * np.hanning(len(half)))) ** 2
    hz = sr / len(half)
    assert 750 % hz == 0
    return 10 * np.log10(spec[int(1250 / hz)] / spec[int(750 / hz)])


def test_shift_frequency_rejects_the_image():
    """a 1 kHz sine shifted by +250 Hz: 1250 Hz, and next to nothing at the image, 750 Hz -- as little as the fp64 restatement leaves, less 6 dB"""
    n, sr = 9600, 48000.0
    x = R1.sine(1, n, 1000.0)
    shift = np.full(n, 250.0, F32)
    got = shift_frequency(x, sr, shift)[0]
    truth = R.shift_frequency(x, sr, shift, dtype=F64)[0]
    spec = np.abs(np.fft.rfft(got[n // 2:].astype(F64) * np.hanning(n - n // 2)))
    assert int(np.argmax(spec)) * sr / (n - n // 2) == 1250.0
    want_db, got_db = rejection_db(truth, sr), rejection_db(got, sr)
    print("image rejection: %.2f dB on the device, %.2f dB in the fp64 restatement" % (got_db, want_db))
    assert want_db > 30.0
    assert got_db >= want_db - 6.0
