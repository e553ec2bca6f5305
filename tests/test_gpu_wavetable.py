"""flan::Wavetable on the MI355X (flan_amd/csrc/wavetable.hip): the table construction against the fp64 truth, the synthesis against the
vectors the reference's own WDL_Resampler made (tests/golden/ref_made/wdl_wavetable.npz) and against the Python restatement
(tests/wavetable_reference.py), the in-place edits against their fp64 forms.  DESIGN.md 4.23 lists the measured values.
The run-planner cases (wdl_wavetable_runs.npz) each assert, from the exported run table (flanhip_wavetable_synth_runs), that they take the
path they are named for -- a block cut into pieces by the staged window, by the output cap, by both; several channels per workgroup in more
than one group -- and are held to bit identity like the others.

Resample: rotations equal the truth's exactly (test_wavetable_reference.py holds the decision margins that allow it); the relative-max error
of a waveform is at most 4 x the single-precision stand-in's on the same waveform, with a floor of 4 fp32 ulp (2^-22).
Measured on the device: the worst waveform reaches 0.40 of its bound at W = 64, 0.31 at W = 256, 0.33 at W = 2048 and 0.29 at W = 8192
(n = 16384: 3.9e-7 against the stand-in's 3.4e-7); the largest error of the W <= 2048 cases is 3.1e-7 (W = 256, n = 255; stand-in 3.2e-7).
Per waveform the kernel's error is between 0.5 and 1.6 times the stand-in's."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import wavetable_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
RESAMPLE_FACTOR, RESAMPLE_FLOOR = 4.0, 2.0 ** -22
# synthesis against the reference-made outputs / the restatement: relative rms error, and max abs error / max |y|.  Measured on the first
# run on the device: every one of the 15 fixture cases and of the 20 random shapes bit-identical (0 samples differ), so both are 0
REL_RMS_BOUND = 0.0
REL_MAX_BOUND = 0.0

CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)
RUN_IDS = [c["name"] for c in RUN_CASES]
RUN_OUTPUTS = 2048                                                 # wavetable.hip's output frames per run


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


# ---------------------------------------------------------------------------------------------------------------
# table construction

_resample_cache = {}


def resample_case(W):
    """the shared case of a wavelength, its truth and stand-in, and the device's table (computed once)"""
    if W not in _resample_cache:
        audio, starts = R.resample_case(W)
        truth, rot, _, _ = R.build_table(audio.astype(np.float64), starts, W)
        standin = R.build_table(audio, starts, W, R.resample_standin)[0]
        table, got_rot = fa.wavetable_resample(audio, starts, W)
        _resample_cache[W] = dict(audio=audio, starts=starts, truth=truth, rot=rot, standin=standin, table=table, got_rot=got_rot)
    return _resample_cache[W]


def check_resample(W, starts, truth, rot, standin, table, got_rot):
    assert table.shape == truth.shape and not np.any(np.isnan(table))
    assert np.array_equal(got_rot, rot), "rotations differ from the truth's"
    worst = 0.0
    for c, s in enumerate(starts):
        for w in range(table.shape[1] // W):
            sl = slice(w * W, (w + 1) * W)
            n = int(s[w + 1]) - int(s[w]) if w + 1 < len(s) else 0
            if n <= 0:
                assert not np.any(table[c, sl]), "a slot no waveform fills must stay 0"
                continue
            scale = np.max(np.abs(truth[c, sl]))
            err = np.max(np.abs(table[c, sl].astype(np.float64) - truth[c, sl])) / scale
            own = np.max(np.abs(standin[c, sl].astype(np.float64) - truth[c, sl])) / scale
            bound = max(RESAMPLE_FACTOR * own, RESAMPLE_FLOOR)
            print("W=%d c=%d n=%d: rel max %.3e (stand-in %.3e, bound %.3e)" % (W, c, n, err, own, bound))
            worst = max(worst, err / bound)
            assert err <= bound, (W, c, n, err, own)
    print("W=%d: worst error / bound = %.3f" % (W, worst))


@pytest.mark.parametrize("W", R.RESAMPLE_W)
def test_resample_against_the_truth(W):
    k = resample_case(W)
    check_resample(W, k["starts"], k["truth"], k["rot"], k["standin"], k["table"], k["got_rot"])


def test_resample_long_waveforms():
    """n above 4096 keeps its twiddles in the workspace, W = 8192 is the largest inverse: n = 16384 (the limit), 5000 and 4097"""
    W, frames = 8192, 17000
    rng = np.random.default_rng(5)
    t = np.arange(frames) / 48000.0
    audio = np.array([0.5 * np.sin(2 * np.pi * 217.3 * t + 0.3) + 0.2 * np.sin(2 * np.pi * 1303.8 * t), 0.3 * rng.standard_normal(frames)], F32)
    starts = [[7, 7 + 16384], [0, 5000, 9097, 9197]]
    truth, rot, margins, maxima = R.build_table(audio.astype(np.float64), starts, W)
    assert np.all(margins >= 1e-4 * maxima)
    standin = R.build_table(audio, starts, W, R.resample_standin)[0]
    table, got_rot = fa.wavetable_resample(audio, starts, W)
    check_resample(W, starts, truth, rot, standin, table, got_rot)


def test_resample_host_and_device_forms_are_bit_identical_and_repeat():
    dev = torch.device("cuda", 0)
    for W in (64, 2048):
        k = resample_case(W)
        audio, starts = k["audio"], k["starts"]
        ch, n = audio.shape
        slots = fa.wavetable_slots(starts)
        d_x = torch.from_numpy(audio).to(dev)
        d_table = torch.full((ch, slots * W), float("nan"), dtype=torch.float32, device=dev)
        d_rot = torch.full((ch, slots), -1, dtype=torch.int32, device=dev)
        d_ws = torch.full((max(fa.wavetable_resample_workspace_bytes(ch, n, starts, W), 16),), 0xFF, dtype=torch.uint8, device=dev)
        fa.wavetable_resample_dev(d_x, ch, n, starts, W, d_table, d_rot, d_ws)
        torch.cuda.synchronize()
        assert np.array_equal(d_table.cpu().numpy().view(np.uint32), k["table"].view(np.uint32)), W
        assert np.array_equal(d_rot.cpu().numpy(), k["got_rot"]), W
        d_table.fill_(float("nan"))
        fa.wavetable_resample_dev(d_x, ch, n, starts, W, d_table, None, d_ws)          # the rotations are optional
        torch.cuda.synchronize()
        assert np.array_equal(d_table.cpu().numpy().view(np.uint32), k["table"].view(np.uint32)), W
        again, again_rot = fa.wavetable_resample(audio, starts, W)
        assert np.array_equal(again.view(np.uint32), k["table"].view(np.uint32)) and np.array_equal(again_rot, k["got_rot"])


# ---------------------------------------------------------------------------------------------------------------
# synthesis

def block_index(c, plan):
    return np.ascontiguousarray(c["index"][:, plan["first_out"]])


def run(c):
    plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    return fa.wavetable_synth(c["table"], c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], block_index(c, plan), c["smooth"])


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_synth_against_the_reference_made_output(c):
    y = run(c)
    assert y.shape == c["out"].shape and not np.any(np.isnan(y))
    rel_rms, rel_max = R.errors(y, c["out"])
    differ = int(np.sum(y.view(np.uint32) != c["out"].view(np.uint32)))
    print("%s: rel_rms=%.3e rel_max=%.3e, %d of %d samples differ" % (c["name"], rel_rms, rel_max, differ, y.size))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)


@pytest.mark.parametrize("seed", range(20))
def test_synth_random_shapes_against_the_restatement(seed):
    table, W, slots, frames, g, freq, ratio, smooth = R.random_synth_case(seed)         # (shared with the planner tests of test_wavetable_capi.py)
    blocks = R.synth_plan(frames, 48000.0, W, g, freq)
    first = np.array([b["first_out"] for b in blocks])
    index = np.ascontiguousarray(np.tile((ratio[first] * F32(slots - 1)).astype(F32), (table.shape[0], 1)))
    want = R.synth(table, W, 48000.0, frames, g, freq, index, smooth, blocks=blocks)
    y = fa.wavetable_synth(table, W, 48000.0, frames, g, freq, index, smooth)
    rel_rms, rel_max = R.errors(y, want)
    print("seed %d: W=%d ch=%d g=%d frames=%d blocks=%d smooth=%d  rel_rms=%.3e rel_max=%.3e" % (
        seed, W, table.shape[0], g, frames, len(blocks), smooth, rel_rms, rel_max))
    assert rel_rms <= REL_RMS_BOUND and rel_max <= REL_MAX_BOUND, (rel_rms, rel_max)


def test_synth_channels_are_independent():
    for name in ("f100", "fsweep", "w2048"):
        c = CASES[IDS.index(name)]
        y = run(c)
        plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
        idx = block_index(c, plan)
        for k in range(c["table"].shape[0]):
            mono = fa.wavetable_synth(c["table"][k:k + 1], c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], idx[k:k + 1], c["smooth"])
            assert np.array_equal(y[k].view(np.uint32), mono[0].view(np.uint32)), (name, k)


def test_synth_host_and_device_forms_are_bit_identical():
    dev = torch.device("cuda", 0)
    for name in ("f1027p5", "fsweep", "f0", "unsmooth", "w2048"):
        c = CASES[IDS.index(name)]
        y_host = run(c)
        assert np.array_equal(y_host.view(np.uint32), run(c).view(np.uint32)), name          # two runs
        plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
        idx = block_index(c, plan)
        ch = c["table"].shape[0]
        slots = c["table"].shape[1] // c["W"]
        d_table = torch.from_numpy(c["table"]).to(dev)
        d_out = torch.full((ch, c["out_frames"]), float("nan"), dtype=torch.float32, device=dev)
        d_ws = torch.full((fa.wavetable_synth_workspace_bytes(ch, c["out_frames"], c["sr"], c["W"], c["g"], c["freq"]),), 0xFF, dtype=torch.uint8, device=dev)
        fa.wavetable_synth_dev(d_table, ch, slots, c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], idx, c["smooth"], d_out, d_ws)
        torch.cuda.synchronize()
        assert np.array_equal(y_host.view(np.uint32), d_out.cpu().numpy().view(np.uint32)), name


# ---------------------------------------------------------------------------------------------------------------
# the run planner's paths (wdl_wavetable_runs.npz)

def tables(c):
    """( the block plan, the run table ) of a case as the launch computes them"""
    args = (c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    return fa.wavetable_synth_plan(*args), fa.wavetable_synth_runs(*args, c["table"].shape[0])


def pieces(r, b):
    """the runs that block b was cut into: their indices, none if the block lies whole in a run"""
    ks = [k for k in range(r["first_out"].size) if r["first_block"][k] == b and r["num_blocks"][k] == 1]
    return ks if len(ks) > 1 else []


def path_pieces(c, ideal, ratio, per_block):
    p, r = tables(c)
    assert np.all(p["ideal"] == ideal) and ratio(p["ratio"])
    full = [b for b in range(p["num_out"].size) if p["num_out"][b] >= c["g"]]
    assert len(full) >= 2
    for b in full:                                                           # every full block is cut, by the window (no piece reaches the output cap)
        ks = pieces(r, b)
        assert per_block(len(ks)), (b, ks)
        assert [int(r["j0"][k]) for k in ks] == list(np.cumsum([0] + [int(r["num_out"][k]) for k in ks[:-1]])) and r["j0"][ks[1]] > 0
        assert all(r["num_out"][k] < RUN_OUTPUTS for k in ks)


def path_outputs_and_window(c):
    p, r = tables(c)
    assert np.all(p["ideal"] == 0)
    ks = pieces(r, 0)
    assert len(ks) >= 3
    inner = [int(r["num_out"][k]) for k in ks[:-1]]                           # every piece but the block's last was closed by a limit
    assert RUN_OUTPUTS in inner and any(v < RUN_OUTPUTS for v in inner), inner           # the output cap, and the window before the cap


def path_groups(c):
    p, r = tables(c)
    assert c["table"].shape[0] == 7 and (r["channels_per_group"], r["groups"]) == (4, 2)        # groups of 4 and 3 channels
    assert r["first_out"].size >= p["num_out"].size - 2                      # a table per block


RUN_PATHS = {
    "piece_window": lambda c: path_pieces(c, 0, lambda ratio: np.all((ratio > 13.0) & (ratio < 13.1)), lambda pieces: pieces >= 2),
    "piece_ratio32": lambda c: path_pieces(c, 1, lambda ratio: np.all(ratio == 32.0), lambda pieces: pieces == 3),
    "piece_outputs_and_window": path_outputs_and_window,
    "groups": path_groups,
}

_device_outputs = {}


def device_output(c):
    """a run-planner case's output in device form, into an output pre-filled with NaN over a workspace pre-filled with 0xFF; computed once"""
    if c["name"] not in _device_outputs:
        dev = torch.device("cuda", 0)
        plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
        ch, slots = c["table"].shape[0], c["table"].shape[1] // c["W"]
        d_table = torch.from_numpy(c["table"]).to(dev)
        d_out = torch.full((ch, c["out_frames"]), float("nan"), dtype=torch.float32, device=dev)
        d_ws = torch.full((fa.wavetable_synth_workspace_bytes(ch, c["out_frames"], c["sr"], c["W"], c["g"], c["freq"]),), 0xFF, dtype=torch.uint8, device=dev)
        fa.wavetable_synth_dev(d_table, ch, slots, c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], block_index(c, plan), c["smooth"], d_out, d_ws)
        torch.cuda.synchronize()
        _device_outputs[c["name"]] = d_out.cpu().numpy()
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


@pytest.mark.parametrize("c", RUN_CASES, ids=RUN_IDS)
def test_run_case_channels_runs_and_forms_are_bit_identical(c):
    y = device_output(c)
    bits = y.view(np.uint32)
    plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    idx = block_index(c, plan)
    for k in range(c["table"].shape[0]):                                     # a channel does not depend on the group it is walked in
        mono = fa.wavetable_synth(c["table"][k:k + 1], c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], idx[k:k + 1], c["smooth"])
        assert np.array_equal(bits[k], mono[0].view(np.uint32)), (c["name"], k)
    assert np.array_equal(bits, run(c).view(np.uint32)), c["name"]           # the host form
    assert np.array_equal(bits, run(c).view(np.uint32)), c["name"]           # and again


# ---------------------------------------------------------------------------------------------------------------
# the in-place edits, on the W = 256 table

def edit_table():
    W = 256
    table = resample_case(W)["table"].copy()
    table[0, W:2 * W] *= F32(0.0004 / np.max(np.abs(table[0, W:2 * W])))          # a slot below the 0.001 threshold
    return table, W


def test_normalize():
    table, W = edit_table()
    got = fa.wavetable_edit(table, W, fa.WT_NORMALIZE)
    assert np.array_equal(got.view(np.uint32), R.normalize(table, W).view(np.uint32))
    assert np.array_equal(got[0, W:2 * W].view(np.uint32), table[0, W:2 * W].view(np.uint32))         # below 0.001: untouched
    assert np.max(np.abs(got[0, :W])) == 1.0


def test_remove_dc():
    table, W = edit_table()
    got = fa.wavetable_edit(table, W, fa.WT_REMOVE_DC).astype(np.float64)
    want = R.remove_dc(table, W)
    # a W-term fp32 sum in any order is within W 2^-24 max |s| of the exact one
    bound = W * 2.0 ** -24 * np.max(np.abs(table.reshape(-1, W)), axis=1, keepdims=True)
    err = np.abs(got - want).reshape(-1, W)
    filled = bound[:, 0] > 0
    print("remove_dc: worst error / bound = %.3e" % np.max(err[filled] / bound[filled]))
    assert np.all(err <= bound)


@pytest.mark.parametrize("fade_frames", [1, 2, 17, 100, 200])
def test_fades(fade_frames):
    """the fade factor is off by a few ulp of sinf (<= 2.4e-7) plus one rounding: within 1e-6 |s| of the fp64 product.  remove_jumps forms
    ( s - mid ) * fade + mid: 3.6e-7 | s - mid | for the difference, the factor and the product, 6e-8 | result | for the sum"""
    table, W = edit_table()
    t64 = table.astype(np.float64)
    got = fa.wavetable_edit(table, W, fa.WT_ADD_FADES, fade_frames)
    want = R.add_fades(table, W, fade_frames)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-6 * np.abs(t64))
    jumps = fa.wavetable_edit(table, W, fa.WT_REMOVE_JUMPS, fade_frames)
    want_j = R.remove_jumps(table, W, fade_frames)
    rows = t64.reshape(-1, W)
    mid = ((rows[:, 0] + rows[:, W - 1]) / 2.0)[:, None]
    bound = 1e-6 * (np.abs(rows - mid) + np.abs(want_j.reshape(-1, W)))
    if fade_frames > W // 2:
        bound = 2 * bound                                                    # the two edges overlap: a sample is faded twice
    assert np.all(np.abs(jumps.astype(np.float64).reshape(-1, W) - want_j.reshape(-1, W)) <= bound)
    touched = np.any((got.view(np.uint32) != table.view(np.uint32)).reshape(-1, W), axis=0)
    edge = min(fade_frames - 1, W)
    assert not np.any(touched[edge:W - edge])                                # fade_frames 1 touches nothing, 2 one frame per edge
    if fade_frames == 1:
        assert np.array_equal(got.view(np.uint32), table.view(np.uint32)) and np.array_equal(jumps.view(np.uint32), table.view(np.uint32))
    if fade_frames == 2:
        assert touched[0] and touched[W - 1] and np.sum(touched) == 2
