"""Audio::repitch on the MI355X (flan_amd/csrc/repitch.hip) against the vectors the reference's own WDL_Resampler made
(tests/golden/ref_made/wdl_repitch.npz) and against the Python restatement (tests/repitch_reference.py).
Bounds: DESIGN.md 4.13 lists the measured values they are set from (<= 30 % above).

The run-planner cases (wdl_repitch_runs.npz) each assert, from the exported run table (flanhip_audio_repitch_runs), that they take the path
they are named for -- taps from global memory, runs closed by the staged window, several channels per workgroup with a ragged last group --
and are held to the same bounds.  Measured on the device: six of the seven bit-identical to the reference-made output; global_3p9 (1 ch x
13000, g = 1600, factor 3.9) 2.541e-9 rms / 3.380e-8 max with 10 of 3693 samples differing, which is to every digit what the restatement gives on
the CPU with position="fma" against the same output: the one-rounding position difference of fma( j, ratio, fracpos ), inside the bounds.  The
same input at g = 1500 (staged taps) against the restatement: 2.466e-9 / 3.380e-8; at g = 1600 (global taps): 2.541e-9 / 3.380e-8."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import repitch_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
# against the reference-made outputs / the restatement: relative rms error, and max abs error / max |y|
REL_RMS_BOUND = 2.7e-9          # set from 2.142e-9 (random shape 16: 2 ch x 2693, g = 6000, against the restatement); global_3p9 reaches 2.541e-9
REL_MAX_BOUND = 3.9e-8          # set from 3.061e-8 (the same shape: single samples one fp32 ulp away); global_3p9 reaches 3.380e-8
# (the 21 fixture cases: 20 bit-identical to the reference-made output, n20 with 1 sample of 69 differing, 1.4e-15 / 3.3e-15)

CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)
RUN_IDS = [c["name"] for c in RUN_CASES]
WINDOW_FLOATS, RUN_OUTPUTS, TAPS, PRELUDE = 6144, 2048, 64, 31     # repitch.hip's staged window and block cap; the resampler's taps and leading zeros


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def case(name):
    return CASES[IDS.index(name)]


def run(c):
    return fa.audio_repitch(c["x"], c["sr"], c["inv"], c["g"], c["quality"])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_against_the_reference_made_output(c):
    y = run(c)
    assert y.shape == c["out"].shape
    rel_rms, rel_max = R.errors(y, c["out"])
    differ = int(np.sum(y.view(np.uint32) != c["out"].view(np.uint32)))
    print("%s: rel_rms=%.3e rel_max=%.3e, %d of %d samples differ" % (c["name"], rel_rms, rel_max, differ, y.size))
    if c["quality"] == R.UNINTERPOLATED:
        assert differ == 0                                                 # copies of input samples
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)
    reached = c["blocks"] * c["g"]
    assert not np.any(y[:, reached:])                                      # what no block reaches stays 0


def test_host_and_device_forms_are_bit_identical():
    dev = torch.device("cuda", 0)
    for name in ("down0p7", "sweep", "u_up1p5", "zero"):
        c = case(name)
        ch, n = c["x"].shape
        y_host = run(c)
        d_x = torch.from_numpy(c["x"]).to(dev)
        d_out = torch.empty((ch, c["out_frames"]), dtype=torch.float32, device=dev)
        d_out.fill_(float("nan"))
        d_ws = torch.empty(fa.audio_repitch_workspace_bytes(n, c["sr"], c["inv"], c["g"], c["quality"]), dtype=torch.uint8, device=dev)
        d_ws.fill_(0xFF)                                                   # no reliance on zeroed workspace
        fa.audio_repitch_dev(d_x, ch, n, c["sr"], c["inv"], c["g"], c["quality"], d_out, d_ws)
        torch.cuda.synchronize()
        y_dev = d_out.cpu().numpy()
        assert np.array_equal(y_host.view(np.uint32), y_dev.view(np.uint32)), name


def test_two_runs_are_bit_identical():
    for name in ("p8_gcd5", "sweep"):
        a, b = run(case(name)), run(case(name))
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_channels_are_independent():
    for name in ("down0p7", "p8_gcd5", "u_down0p7"):
        c = case(name)
        y = run(c)
        for k in range(3):
            mono = fa.audio_repitch(c["x"][k:k + 1], c["sr"], c["inv"], c["g"], c["quality"])
            assert np.array_equal(y[k].view(np.uint32), mono[0].view(np.uint32)), (name, k)


@pytest.mark.parametrize("factor,peak_hz", [(1.5, 1500.0), (0.7, 700.0)])
def test_a_sine_moves_to_factor_times_its_frequency(factor, peak_hz):
    sr, n, g = 48000.0, 12000, 48                                          # 0.25 s of 1 kHz
    x = (0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(n) / sr)).astype(F32)[None, :]
    inv = R.invert(np.full(R.factor_count(n, g), factor, F32))
    y = fa.audio_repitch(x, sr, inv, g)
    blocks = len(R.plan(n, sr, inv, g))
    body = y[0, :min(y.shape[1], blocks * g)].astype(np.float64)
    spectrum = np.abs(np.fft.rfft(body * np.hanning(body.size)))
    got_hz = np.argmax(spectrum) * sr / body.size
    print("factor %g: peak at %.1f Hz (bin width %.1f Hz)" % (factor, got_hz, sr / body.size))
    assert abs(got_hz - peak_hz) <= sr / body.size
    # against the smooth fp64 truth: no worse than twice the restatement's own error on the same input (they differ in table rounding only)
    truth = R.smooth_truth(x, sr, factor, y.shape[1])[:, :body.size]
    own_rms, own_max = R.errors(R.repitch(x, sr, inv, g)[:, :body.size], truth)
    rel_rms, rel_max = R.errors(y[:, :body.size], truth)
    print("factor %g: against the smooth truth rel_rms=%.3e rel_max=%.3e (the restatement: %.3e, %.3e)" % (factor, rel_rms, rel_max, own_rms, own_max))
    assert rel_rms <= 2 * own_rms and rel_max <= 2 * own_max


@pytest.mark.parametrize("seed", range(20))
def test_random_shapes_against_the_restatement(seed):
    x, sr, inv, g, quality = R.random_case(seed)               # (shared with the planner tests of test_repitch_capi.py)
    want = R.repitch(x, sr, inv, g, quality)
    y = fa.audio_repitch(x, sr, inv, g, quality)
    assert y.shape == want.shape
    rel_rms, rel_max = R.errors(y, want)
    print("seed %d: ch=%d n=%d g=%d q=%d -> %d frames  rel_rms=%.3e rel_max=%.3e" % (seed, x.shape[0], x.shape[1], g, quality, y.shape[1], rel_rms, rel_max))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)


# ---------------------------------------------------------------------------------------------------------------
# the run planner's paths (wdl_repitch_runs.npz)

def run_case(name):
    return RUN_CASES[RUN_IDS.index(name)]


def tables(c, g=None, inv=None):
    """( the block plan, the run table ) of a case as the launch computes them"""
    ch, n = c["x"].shape
    g, inv = g or c["g"], c["inv"] if inv is None else inv
    return fa.audio_repitch_plan(n, c["sr"], inv, g, c["quality"]), fa.audio_repitch_runs(n, c["sr"], inv, g, ch, c["quality"])


def same_table(p, a, b):
    return all(p[key][a] == p[key][b] for key in ("filtpos", "oversize", "ideal"))


def closed_by(p, r, g):
    """why every run but the last ends where it does: "table", "cap" (2048 / g blocks) or "window" """
    why = []
    for k in range(r["first_block"].size - 1):
        a, nxt = int(r["first_block"][k]), int(r["first_block"][k + 1])
        why.append("table" if not same_table(p, a, nxt) else "cap" if r["num_blocks"][k] == max(RUN_OUTPUTS // g, 1) else "window")
    return why


def data_under_every_tap(p, b, g, n):
    """every tap of every output of block b reads an input sample, none of the zeros around the input"""
    pos = float(p["fracpos"][b])
    for _ in range(g - 1):
        pos += float(p["ratio"][b])
    return p["offset"][b] + int(p["fracpos"][b]) >= PRELUDE and p["offset"][b] + int(pos) + TAPS <= PRELUDE + n


def path_global(c, ideal):
    p, r = tables(c)
    assert r["first_block"].size >= 2 and np.all(r["win_len"] == 0)        # every run reads its taps from global memory
    assert np.all(p["offset"][1:] > 0) and np.all(p["ideal"] == ideal)
    assert any(data_under_every_tap(p, b, c["g"], c["x"].shape[1]) for b in range(1, p["offset"].size))


def path_window(c, min_blocks):
    p, r = tables(c)
    why = closed_by(p, r, c["g"])
    assert why and why[0] == "window", why                                 # neither a table change nor the block cap ended the first run
    assert r["num_blocks"][0] >= min_blocks and np.all(r["win_len"] > 0)
    assert r["win_start"][1] > WINDOW_FLOATS // 2                          # the next run's window starts far from 0


def path_step(c):
    p, r = tables(c)
    why = closed_by(p, r, c["g"])
    assert "table" in why and "cap" in why, why
    assert set(p["ideal"].tolist()) == {0, 1}                              # the fracpos quantisation at an ideal block's end, then a table that is not


def path_groups(c, runs, cpw, groups, last):
    p, r = tables(c)
    ch = c["x"].shape[0]
    assert runs(r["first_block"].size), r["first_block"].size
    assert (r["channels_per_group"], r["groups"]) == (cpw, groups) and ch - (groups - 1) * cpw == last


RUN_PATHS = {
    "global_3p9": lambda c: path_global(c, 0),
    "global_ideal4": lambda c: path_global(c, 1),
    "window_cut": lambda c: path_window(c, 2),
    "window_cut_g1": lambda c: path_window(c, 1501),
    "step_3p9": path_step,
    "groups_sweep": lambda c: path_groups(c, lambda runs: runs > 1, 6, 3, 1),
    "groups_small": lambda c: path_groups(c, lambda runs: runs == 1, 2, 3, 1),
}

_device_outputs = {}


def device_form(x, sr, inv, g, quality):
    """the device form into an output pre-filled with NaN, over a workspace pre-filled with 0xFF"""
    dev = torch.device("cuda", 0)
    ch, n = x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_out = torch.full((ch, fa.audio_repitch_out_frames(inv, g)), float("nan"), dtype=torch.float32, device=dev)
    d_ws = torch.full((fa.audio_repitch_workspace_bytes(n, sr, inv, g, quality),), 0xFF, dtype=torch.uint8, device=dev)
    fa.audio_repitch_dev(d_x, ch, n, sr, inv, g, quality, d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def device_output(c):
    """a run-planner case's output in device form, computed once"""
    if c["name"] not in _device_outputs:
        _device_outputs[c["name"]] = device_form(c["x"], c["sr"], c["inv"], c["g"], c["quality"])
    return _device_outputs[c["name"]]


def test_every_run_case_has_its_path():
    assert sorted(RUN_PATHS) == sorted(RUN_IDS)


@pytest.mark.parametrize("c", RUN_CASES, ids=RUN_IDS)
def test_run_case_takes_the_path_it_is_named_for(c):
    RUN_PATHS[c["name"]](c)


@pytest.mark.parametrize("c", RUN_CASES, ids=RUN_IDS)
def test_run_case_against_the_reference_made_output(c):
    y = device_output(c)
    assert y.shape == c["out"].shape and not np.any(np.isnan(y))
    rel_rms, rel_max = R.errors(y, c["out"])
    differ = int(np.sum(y.view(np.uint32) != c["out"].view(np.uint32)))
    print("%s: rel_rms=%.3e rel_max=%.3e, %d of %d samples differ" % (c["name"], rel_rms, rel_max, differ, y.size))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)
    reached = c["blocks"] * c["g"]
    assert not np.any(y[:, reached:])                                      # what no block reaches stays 0


@pytest.mark.parametrize("c", RUN_CASES, ids=RUN_IDS)
def test_run_case_channels_runs_and_forms_are_bit_identical(c):
    y = device_output(c)
    bits = y.view(np.uint32)
    for k in range(c["x"].shape[0]):                                       # a channel does not depend on the group it is walked in
        mono = fa.audio_repitch(c["x"][k:k + 1], c["sr"], c["inv"], c["g"], c["quality"])
        assert np.array_equal(bits[k], mono[0].view(np.uint32)), (c["name"], k)
    host = run(c)
    assert np.array_equal(bits, host.view(np.uint32)), c["name"]           # the host form
    assert np.array_equal(bits, run(c).view(np.uint32)), c["name"]         # and again


def test_staged_and_global_taps_agree_with_the_restatement_equally():
    """global_3p9's input and factor at g = 1600 (a block's window is past the staging buffer: global-memory taps) and at g = 1500
    (span + 68 <= 6144: staged), each against the restatement under the bounds of this file"""
    c = run_case("global_3p9")
    x, n = c["x"], c["x"].shape[1]
    errors = {}
    for g, staged in ((1600, False), (1500, True)):
        inv = R.invert(np.full(R.factor_count(n, g), 3.9, F32))
        p, r = tables(c, g, inv)
        assert np.all((r["win_len"] > 0) == staged) and p["offset"].size >= 2, (g, r["win_len"])
        if not staged:
            assert np.array_equal(inv, c["inv"])
        y = device_form(x, c["sr"], inv, g, c["quality"])
        errors[g] = R.errors(y, R.repitch(x, c["sr"], inv, g, c["quality"]))
    print("global taps (g 1600): rel_rms=%.3e rel_max=%.3e   staged (g 1500): rel_rms=%.3e rel_max=%.3e" % (errors[1600] + errors[1500]))
    for g in errors:
        assert errors[g][0] <= REL_RMS_BOUND and errors[g][1] <= REL_MAX_BOUND, (g, errors[g])
