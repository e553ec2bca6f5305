"""flan::Wavetable's C ABI (include/flanhip.h, flan_amd/csrc/wavetable.hip) without a device: symbols, the host-only entry points (snap,
starts, table index, every field of the synthesis plan) against the restatement bit for bit, refusals, and the invariants of the runs the
synthesis launch cuts that plan into (the exported run table, over the fixture cases, the random seeds of the device tests and the
run-planner cases of wdl_wavetable_runs.npz)."""
import ctypes
import os

import numpy as np
import pytest

import wavetable_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_wavetable_snap", "flanhip_wavetable_starts", "flanhip_wavetable_table_index", "flanhip_wavetable_slots",
           "flanhip_wavetable_resample_workspace_bytes", "flanhip_wavetable_resample_dev", "flanhip_wavetable_resample",
           "flanhip_wavetable_synth_plan", "flanhip_wavetable_synth_runs", "flanhip_wavetable_synth_workspace_bytes", "flanhip_wavetable_synth_dev", "flanhip_wavetable_synth",
           "flanhip_wavetable_edit_dev", "flanhip_wavetable_edit"]
CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)
RUN_IDS = [c["name"] for c in RUN_CASES]
WINDOW_FLOATS, RUN_OUTPUTS = 6144, 2048                            # the limits wavetable.hip cuts its runs by
PLAN_KEYS = ("offset", "fracpos", "ratio", "filtpos", "oversize", "ideal", "first_out", "num_out", "wanted", "in_start")


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_wavetable_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
        assert name + "(" in header, name
    for name in ("wavetable_snap", "wavetable_starts", "wavetable_table_index", "wavetable_resample", "wavetable_resample_dev", "wavetable_synth_plan", "wavetable_synth_runs",
                 "wavetable_synth", "wavetable_synth_dev", "wavetable_edit", "wavetable_edit_dev"):
        assert callable(getattr(fa, name))


def test_snap_equals_the_restatement():
    rng = np.random.default_rng(11)
    rows = [np.sin(2 * np.pi * (np.arange(300) + 0.3) / 41).astype(F32), (0.3 * rng.standard_normal(300)).astype(F32), np.full(300, 0.5, F32),
            (np.abs(rng.standard_normal(300)) + 0.01).astype(F32)]             # the last two never cross zero: the fallback
    for row in rows:
        for frame in (0, 1, 57, 150, 298, 299):
            for distance in (0, 1, 5, 40, 1000, -3):
                for height in (0.0, float(row[max(frame - 20, 0)])):
                    assert fa.wavetable_snap(row, frame, height, distance) == R.snap(row, frame, height, distance), (frame, distance, height)


def test_starts_equal_the_restatement():
    rng = np.random.default_rng(12)
    n = 3000
    tone = np.sin(2 * np.pi * (np.arange(n) + 0.3) / 100).astype(F32)
    noisy = (tone + 0.2 * rng.standard_normal(n)).astype(F32)
    locals_ = np.where(rng.uniform(size=n // 128 + 1) < 0.3, 0, rng.uniform(80, 130, n // 128 + 1)).astype(F32)
    for row in (tone, noisy):
        for snap_mode in (R.SNAP_NONE, R.SNAP_ZERO, R.SNAP_LEVEL):
            for pitch_mode, loc, glob in ((R.PITCH_NONE, None, 0), (R.PITCH_GLOBAL, None, 97), (R.PITCH_LOCAL, locals_, 101), (R.PITCH_LOCAL, locals_, -1),
                                          (R.PITCH_LOCAL, locals_[:5], 0), (R.PITCH_LOCAL, np.zeros(0, F32), 50)):
                for snap_ratio, fixed in ((0.3, 256), (0.9, 77), (0.01, 2999), (0.5, 5000)):
                    got = fa.wavetable_starts(row, loc, glob, snap_mode, pitch_mode, snap_ratio, fixed)
                    want = R.starts(row, [] if loc is None else loc, glob, snap_mode, pitch_mode, snap_ratio, fixed)
                    assert np.array_equal(got, want), (snap_mode, pitch_mode, glob, snap_ratio, fixed)


def test_starts_refusals():
    row = np.sin(np.arange(500) / 7.0).astype(F32)
    count = ctypes.c_int64(0)
    L = fa.lib
    call = lambda row_p, n, glob, snap, pitch, ratio, fixed: L.flanhip_wavetable_starts(          # noqa: E731
        row_p, n, None, 0, glob, snap, pitch, ratio, fixed, None, None, 0, ctypes.cast(ctypes.byref(count), ctypes.c_void_p))
    assert call(p(row), 500, 0, 0, 0, 0.3, 256) == fa.OK and count.value == 2
    assert call(None, 500, 0, 0, 0, 0.3, 256) == fa.ERR_INVALID_ARG
    assert call(p(row), 0, 0, 0, 0, 0.3, 256) == fa.ERR_INVALID_ARG
    assert call(p(row), 500, 0, 0, 0, 0.3, 0) == fa.ERR_INVALID_ARG          # fixed_frame < 1 (:145)
    assert call(p(row), 500, 0, 0, 0, 0.0, 256) == fa.ERR_INVALID_ARG        # snap_ratio outside ( 0, .95 ) (:146)
    assert call(p(row), 500, 0, 0, 0, 0.96, 256) == fa.ERR_INVALID_ARG
    assert call(p(row), 500, 0, 0, 0, 0.95, 256) == fa.OK                    # 0.95f is below the double .95 the reference compares with
    assert call(p(row), 500, 0, 3, 0, 0.3, 256) == fa.ERR_INVALID_ARG
    assert call(p(row), 500, 0, 0, 3, 0.3, 256) == fa.ERR_INVALID_ARG
    assert call(p(row), 500, 0, 0, R.PITCH_GLOBAL, 0.3, 256) == fa.ERR_UNSUPPORTED       # a global wavelength of 0: the reference's walk would not end
    assert "below one frame" in fa.last_error()
    out = ctypes.c_int32(0)
    assert L.flanhip_wavetable_snap(p(row), 500, 500, 0.0, 5, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == fa.ERR_INVALID_ARG
    assert L.flanhip_wavetable_snap(p(row), 500, -1, 0.0, 5, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == fa.ERR_INVALID_ARG
    assert L.flanhip_wavetable_snap(None, 500, 5, 0.0, 5, ctypes.cast(ctypes.byref(out), ctypes.c_void_p)) == fa.ERR_INVALID_ARG


def test_table_index_equals_the_restatement():
    rng = np.random.default_rng(13)
    r = np.concatenate([np.linspace(-0.5, 1.5, 401), rng.uniform(0, 1, 200), [0.0, 1.0, 0.11, 0.0604, np.nan, np.inf, -np.inf, 1e30]]).astype(F32)
    for starts in ([10, 110, 310, 610], [0], [0, 999], [5, 300, 610], sorted(rng.integers(0, 1000, 40).tolist())):
        got = fa.wavetable_table_index(starts, 1000, r)
        finite = np.isfinite(r) & (np.abs(r) < 1e6)
        want = np.array([R.table_index(starts, 1000, v) for v in r[finite]], F32)
        assert np.array_equal(got[finite].view(np.uint32), want.view(np.uint32)), starts
        assert got[~finite].tolist() == [0.0, len(starts) - 1, 0.0, len(starts) - 1]          # NaN is 0; what no Frame holds saturates


@pytest.mark.parametrize("c", CASES + RUN_CASES, ids=IDS + RUN_IDS)
def test_synth_plan_equals_the_restatement_and_the_reference(c):
    plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    want = R.synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    assert plan["wanted"].size == c["blocks"]
    for key in PLAN_KEYS:
        assert np.array_equal(plan[key], np.array([b[key] for b in want], plan[key].dtype)), key       # fp64, the same chain of additions: to the bit
    assert np.array_equal(plan["wanted"], c["wanted"]) and np.array_equal(plan["num_out"], c["delivered"])
    assert np.array_equal(plan["in_start"], np.concatenate([[0], np.cumsum(c["wanted"])[:-1]]))
    assert int(plan["first_out"][-1] + plan["num_out"][-1]) == c["out_frames"]                        # every output frame belongs to a block


def test_synth_plan_on_shapes_of_its_own():
    for W, g, frames, freq in ((64, 1, 300, [1027.5]), (128, 7, 1000, np.linspace(50, 4000, 1000)), (64, 480, 3000, [99.75]), (2048, 48, 500, [440.0]),
                               (64, 48, 5000, [1.0])):
        plan = fa.wavetable_synth_plan(frames, 48000.0, W, g, freq)
        want = R.synth_plan(frames, 48000.0, W, g, freq)
        for key in PLAN_KEYS:
            assert np.array_equal(plan[key], np.array([b[key] for b in want], plan[key].dtype)), (W, g, key)


def test_synth_refusals():
    L = fa.lib
    f = np.array([440.0], F32)
    none10 = [None] * 10
    plan = lambda frames, sr, W, g, fp, count: L.flanhip_wavetable_synth_plan(frames, sr, W, g, fp, count, 0, *none10)      # noqa: E731
    assert plan(2400, 48000.0, 64, 48, p(f), 1) > 0
    assert plan(2400, 48000.0, 64, 0, p(f), 1) == fa.ERR_INVALID_ARG         # g < 1: the reference would loop forever
    assert "granularity" in fa.last_error()
    assert plan(2400, 48000.0, 64, -3, p(f), 1) == fa.ERR_INVALID_ARG
    assert plan(0, 48000.0, 64, 48, p(f), 1) == fa.ERR_INVALID_ARG
    assert plan(2400, 0.0, 64, 48, p(f), 1) == fa.ERR_INVALID_ARG
    assert plan(2400, 48000.0, 0, 48, p(f), 1) == fa.ERR_INVALID_ARG
    assert plan(2400, 48000.0, 64, 48, None, 1) == fa.ERR_INVALID_ARG
    assert plan(2400, 48000.0, 64, 48, p(f), 0) == fa.ERR_INVALID_ARG
    nan = np.array([np.nan], F32)
    assert plan(2400, 48000.0, 64, 48, p(nan), 1) == fa.ERR_INVALID_ARG
    high = np.array([750.0 * 40], F32)                                       # a ratio of 40: after its first block the reference reads stale samples
    assert plan(2400, 48000.0, 64, 48, p(high), 1) == fa.ERR_UNSUPPORTED
    assert "stale" in fa.last_error()
    assert fa.wavetable_synth_workspace_bytes(2, 2400, 48000.0, 64, 0, f) == 0
    assert fa.wavetable_synth_workspace_bytes(2, 2400, 48000.0, 64, 48, f) > 0
    table = np.zeros((1, 5 * 64), F32)
    out = np.zeros((1, 2400), F32)
    blocks = plan(2400, 48000.0, 64, 48, p(f), 1)
    index = np.zeros(blocks, F32)
    synth = lambda tp, slots, ip, nb, op: L.flanhip_wavetable_synth(tp, 1, slots, 64, 48000.0, 2400, 48, p(f), 1, ip, nb, 1, op, None)     # noqa: E731
    assert synth(None, 5, p(index), blocks, p(out)) == fa.ERR_INVALID_ARG
    assert synth(p(table), 5, None, blocks, p(out)) == fa.ERR_INVALID_ARG
    assert synth(p(table), 5, p(index), blocks, None) == fa.ERR_INVALID_ARG
    assert synth(p(table), 5, p(index), blocks - 1, p(out)) == fa.ERR_INVALID_ARG          # one index per block of the plan
    index[3] = 4.5
    assert synth(p(table), 5, p(index), blocks, p(out)) == fa.ERR_INVALID_ARG              # an index outside the table
    assert "outside the table" in fa.last_error()
    ws = ctypes.c_void_p(1 << 40)                                            # never dereferenced: the refusals come first
    index[3] = 0
    assert L.flanhip_wavetable_synth_dev(ws, 1, 5, 64, 48000.0, 2400, 48, p(f), 1, p(index), blocks, 1, ws, None, None) == fa.ERR_INVALID_ARG


def test_resample_and_edit_refusals():
    L = fa.lib
    x = np.zeros((1, 1000), F32)
    starts = np.array([0, 100, 300], np.int32)
    counts = np.array([3], np.int64)
    res = lambda xp, W, sp, cp, tp, frames=1000: L.flanhip_wavetable_resample(xp, 1, frames, sp, cp, W, tp, None, None)     # noqa: E731
    table = np.zeros((1, 3 * 8192), F32)
    for W in (100, 96, 32, 16384, 3):                                        # not a power of two, below 64, above 8192
        assert res(p(x), W, p(starts), p(counts), p(table)) == fa.ERR_UNSUPPORTED, W
        assert "power of two" in fa.last_error()
        assert fa.wavetable_resample_workspace_bytes(1, 1000, [starts], W) == 0
    assert res(p(x), 0, p(starts), p(counts), p(table)) == fa.ERR_INVALID_ARG
    assert res(None, 64, p(starts), p(counts), p(table)) == fa.ERR_INVALID_ARG
    assert res(p(x), 64, None, p(counts), p(table)) == fa.ERR_INVALID_ARG
    assert res(p(x), 64, p(starts), None, p(table)) == fa.ERR_INVALID_ARG
    assert res(p(x), 64, p(starts), p(counts), None) == fa.ERR_INVALID_ARG
    assert res(p(x), 64, p(starts), p(counts), p(table), 299) == fa.ERR_INVALID_ARG        # a waveform leaves the source
    zero = np.array([0], np.int64)
    assert res(p(x), 64, p(starts), p(zero), p(table)) == fa.ERR_INVALID_ARG
    long_x = np.zeros((1, 20000), F32)
    long_starts = np.array([0, 16385], np.int32)
    two = np.array([2], np.int64)
    assert res(p(long_x), 8192, p(long_starts), p(two), p(table), 20000) == fa.ERR_UNSUPPORTED
    assert "16384" in fa.last_error()
    assert fa.wavetable_resample_workspace_bytes(1, 20000, [[0, 16384]], 8192) > 0          # the limit itself is served
    assert fa.wavetable_slots([[0, 5, 9], [1, 2]]) == 3
    ws = ctypes.c_void_p(1 << 40)
    assert L.flanhip_wavetable_resample_dev(ws, 1, 1000, p(starts), p(counts), 64, ws, None, None, None) == fa.ERR_INVALID_ARG      # null workspace
    edit = lambda tp, ch, slots, W, mode, fade: L.flanhip_wavetable_edit(tp, ch, slots, W, mode, fade, None)      # noqa: E731
    assert edit(None, 1, 3, 64, 0, 0) == fa.ERR_INVALID_ARG
    assert edit(p(table), 0, 3, 64, 0, 0) == fa.ERR_INVALID_ARG
    assert edit(p(table), 1, 3, 64, 4, 8) == fa.ERR_INVALID_ARG
    assert edit(p(table), 1, 3, 64, fa.WT_ADD_FADES, 0) == fa.ERR_INVALID_ARG


def test_valid_calls_without_a_device_say_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    c = CASES[IDS.index("f1027p5")]
    plan = fa.wavetable_synth_plan(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"])
    index = np.ascontiguousarray(c["index"][:, plan["first_out"]])
    with pytest.raises(fa.FlanHipError) as e:
        fa.wavetable_synth(c["table"], c["W"], c["sr"], c["out_frames"], c["g"], c["freq"], index, c["smooth"])
    assert e.value.code == fa.ERR_NO_DEVICE
    audio, starts = R.resample_case(64)
    with pytest.raises(fa.FlanHipError) as e:
        fa.wavetable_resample(audio, starts, 64)
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.wavetable_edit(c["table"], c["W"], fa.WT_NORMALIZE)
    assert e.value.code == fa.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------
# the runs of the synthesis launch (flanhip_wavetable_synth_runs: the launch's own planner, exported)

def planner_shapes():
    """( id, ch, out_frames, sr, W, g, freq ) of every fixture case, every random seed of the device tests and every run-planner case"""
    shapes = [(c["name"], c["table"].shape[0], c["out_frames"], c["sr"], c["W"], c["g"], c["freq"]) for c in CASES + RUN_CASES]
    for seed in range(20):
        table, W, slots, frames, g, freq, ratio, smooth = R.random_synth_case(seed)
        shapes.append(("seed%d" % seed, table.shape[0], frames, 48000.0, W, g, freq))
    return shapes


SHAPES = planner_shapes()


def block_positions(plan, b):
    """srcpos of every output of block b: the reference's chain of additions from the block's fracpos"""
    pos, out = float(plan["fracpos"][b]), []
    for _ in range(int(plan["num_out"][b])):
        out.append(pos)
        pos += float(plan["ratio"][b])
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_runs_tile_the_output_within_their_limits(shape):
    _, ch, frames, sr, W, g, freq = shape
    plan = fa.wavetable_synth_plan(frames, sr, W, g, freq)
    r = fa.wavetable_synth_runs(frames, sr, W, g, freq, ch)
    first_out, num_out = r["first_out"], r["num_out"].astype(np.int64)
    assert np.all(plan["num_out"] >= 1)                                             # no block without output (DESIGN.md 4.23 says why)
    # the runs' output frames tile [0, out_frames) once, in order
    assert first_out.size >= 1 and first_out[0] == 0 and np.all(num_out >= 1)
    assert np.array_equal(first_out[1:], first_out[:-1] + num_out[:-1]) and first_out[-1] + num_out[-1] == frames
    assert np.all(num_out <= RUN_OUTPUTS)
    assert np.all(r["win_len"] > 0) and np.all(r["win_len"] <= WINDOW_FLOATS)       # always staged: the kernel gives the row form an empty row
    block_of = np.repeat(np.arange(plan["num_out"].size), plan["num_out"])          # the block of every output frame
    block_end = plan["first_out"] + plan["num_out"]
    for k in range(first_out.size):
        a, z = int(first_out[k]), int(first_out[k] + num_out[k]) - 1                # the run's first and last frame
        ba, bz = int(block_of[a]), int(block_of[z])
        assert ba == r["first_block"][k] and bz < r["first_block"][k] + r["num_blocks"][k], k
        assert a - int(plan["first_out"][ba]) == r["j0"][k], k
        if r["j0"][k] > 0 or z + 1 != block_end[bz]:
            assert ba == bz, k                                                      # a piece of a cut block: that block alone
        with_output = [b for b in range(ba, bz + 1) if plan["num_out"][b] > 0]
        for key in ("filtpos", "oversize", "ideal"):
            assert all(plan[key][b] == plan[key][ba] for b in with_output), (k, key)       # one coefficient table per run
        lo, hi = int(r["win_start"][k]), int(r["win_start"][k]) + int(r["win_len"][k])
        for b in with_output:                                                       # the 64 taps of the first and last output of every block's share
            pos = block_positions(plan, b)
            j_first = a - int(plan["first_out"][b]) if b == ba else 0
            j_last = z - int(plan["first_out"][b]) if b == bz else len(pos) - 1
            for j in (j_first, j_last):
                s0 = int(plan["offset"][b]) + int(pos[j])
                assert lo <= s0 and s0 + R.TAPS <= hi, (k, b, j, lo, hi, s0)
    cpw, groups = r["channels_per_group"], r["groups"]
    assert cpw >= 1 and groups * cpw >= ch > (groups - 1) * cpw


def test_channel_groups_cover_every_channel_count():
    c = RUN_CASES[RUN_IDS.index("groups")]
    for ch in range(1, 40):
        r = fa.wavetable_synth_runs(c["out_frames"], c["sr"], c["W"], c["g"], c["freq"], ch)
        cpw, groups = r["channels_per_group"], r["groups"]
        assert 1 <= cpw <= ch and groups * cpw >= ch > (groups - 1) * cpw, (ch, cpw, groups)


def test_runs_refusals_and_counting():
    L = fa.lib
    f = np.array([9803.7], F32)
    none7 = [None] * 7
    runs = lambda frames, g, fp, ch, cpw=None, groups=None: L.flanhip_wavetable_synth_runs(frames, 48000.0, 64, g, fp, 1, ch, 0, *none7, cpw, groups)     # noqa: E731
    cpw, groups = ctypes.c_int(-1), ctypes.c_int64(-1)
    assert runs(1500, 480, p(f), 2, ctypes.byref(cpw), ctypes.byref(groups)) == 7
    assert (cpw.value, groups.value) == (2, 1)
    assert runs(1500, 480, p(f), 2) == 7                                     # everything nullable
    win_len = np.full(2, -1, np.int32)                                       # a capacity below the run count fills that many records
    assert L.flanhip_wavetable_synth_runs(1500, 48000.0, 64, 480, p(f), 1, 2, 2, None, None, None, None, None, None, p(win_len), None, None) == 7
    assert np.all(win_len > 0) and np.all(win_len <= WINDOW_FLOATS)
    assert runs(1500, 480, p(f), 0) == fa.ERR_INVALID_ARG
    assert runs(1500, 480, None, 2) == fa.ERR_INVALID_ARG
    assert runs(1500, 0, p(f), 2) == fa.ERR_INVALID_ARG
    assert runs(0, 480, p(f), 2) == fa.ERR_INVALID_ARG
    high = np.array([750.0 * 40], F32)
    assert runs(1500, 480, p(high), 2) == fa.ERR_UNSUPPORTED                 # the plan's own refusal
