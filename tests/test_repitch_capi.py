"""Audio::repitch's C ABI (include/flanhip.h, flan_amd/csrc/repitch.hip) without a device: symbols, the host plan against the vectors
the reference's own resampler made, refusals, and the invariants of the runs the sinc launch cuts that plan into (the exported run table,
over the fixture cases, the random seeds of the device tests and the run-planner cases of wdl_repitch_runs.npz)."""
import ctypes
import os

import numpy as np
import pytest

import repitch_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_audio_repitch_out_frames", "flanhip_audio_repitch_plan", "flanhip_audio_repitch_runs", "flanhip_audio_repitch_workspace_bytes",
           "flanhip_audio_repitch", "flanhip_audio_repitch_dev"]
CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)
RUN_IDS = [c["name"] for c in RUN_CASES]
WINDOW_FLOATS, RUN_OUTPUTS, TAPS = 6144, 8 * 256, 64               # the limits repitch.hip cuts its runs by


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_repitch_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
    for name in ("audio_repitch", "audio_repitch_dev", "audio_repitch_plan", "audio_repitch_runs", "audio_repitch_out_frames", "audio_repitch_workspace_bytes"):
        assert callable(getattr(fa, name))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name


@pytest.mark.parametrize("case", CASES + RUN_CASES, ids=IDS + RUN_IDS)
def test_out_frames_and_plan_equal_the_references(case):
    n = case["x"].shape[1]
    assert fa.audio_repitch_out_frames(case["inv"], case["g"]) == case["out_frames"]
    p = fa.audio_repitch_plan(n, case["sr"], case["inv"], case["g"], case["quality"])
    assert p["out_frames"] == case["out_frames"]
    assert p["wanted"].size == case["blocks"]
    assert np.array_equal(p["wanted"], case["wanted"])
    want = R.plan(n, case["sr"], case["inv"], case["g"], case["quality"])               # fp64, the same chain of additions: equal to the bit
    for key in ("offset", "fracpos", "ratio", "filtpos", "oversize", "first_out"):
        assert np.array_equal(p[key], np.array([b[key] for b in want], p[key].dtype)), key
    assert np.array_equal(p["ideal"] != 0, np.array([b["ideal"] for b in want], bool))


def test_plan_counts_without_storage():
    c = CASES[IDS.index("sweep")]
    inv = np.ascontiguousarray(c["inv"])
    nout = ctypes.c_int64(0)
    got = fa.lib.flanhip_audio_repitch_plan(4000, c["sr"], inv.ctypes.data_as(ctypes.c_void_p), inv.size, c["g"], 0, 0,
                                            None, None, None, None, None, None, None, None, ctypes.byref(nout))
    assert got == c["blocks"] and nout.value == c["out_frames"]


def test_workspace_bytes_follow_the_layout():
    c = CASES[IDS.index("up1p5")]
    assert fa.audio_repitch_workspace_bytes(1000, c["sr"], c["inv"], c["g"], fa.REPITCH_UNINTERPOLATED) == 64 * 2080 * 8 + 56 * 14
    sinc = fa.audio_repitch_workspace_bytes(1000, c["sr"], c["inv"], c["g"])
    assert sinc >= 64 * 2080 * 8 + 56 * c["blocks"] + 40 and (sinc - 64 * 2080 * 8 - 56 * c["blocks"]) % 40 == 0
    assert fa.audio_repitch_workspace_bytes(0, c["sr"], c["inv"], c["g"]) == 0
    assert fa.audio_repitch_workspace_bytes(1000, c["sr"], c["inv"], c["g"], fa.REPITCH_LINEAR) == 0


def test_out_frames_refusals():
    inv = np.ones(4, np.float32)
    p = inv.ctypes.data_as(ctypes.c_void_p)
    L = fa.lib
    assert L.flanhip_audio_repitch_out_frames(None, 4, 48) == 0
    assert L.flanhip_audio_repitch_out_frames(p, 0, 48) == 0
    assert L.flanhip_audio_repitch_out_frames(p, 4, 0) == 0
    assert L.flanhip_audio_repitch_out_frames(p, 4, 48) == 192


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((1, 100), np.float32)
    inv = np.ones(3, np.float32)
    out = np.zeros((1, 144), np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    L = fa.lib
    assert L.flanhip_audio_repitch(None, 1, 100, 48000.0, p(inv), 3, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, None, 3, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 3, 48, 0, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 0, 100, 48000.0, p(inv), 3, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, -1, 48000.0, p(inv), 3, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 0, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 3, 0, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 0.0, p(inv), 3, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 3, 48, 7, p(out), None) == fa.ERR_INVALID_ARG
    # one factor serves input frames [0, 48): the loop's second block needs factor 1 (in_frame = 85 after the first)
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 1, 48, 0, p(out), None) == fa.ERR_INVALID_ARG
    assert "fewer than the loop needs" in fa.last_error()
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(inv), 3, 48, fa.REPITCH_LINEAR, p(out), None) == fa.ERR_UNSUPPORTED
    assert "Linear" in fa.last_error()
    ws = ctypes.c_void_p(1 << 40)                                        # never dereferenced: the refusals come first
    assert L.flanhip_audio_repitch_dev(None, 1, 100, 48000.0, p(inv), 3, 48, 0, ws, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch_dev(ws, 1, 100, 48000.0, p(inv), 3, 48, 0, ws, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch_dev(ws, 1, 100, 48000.0, p(inv), 3, 48, fa.REPITCH_LINEAR, ws, ws, None) == fa.ERR_UNSUPPORTED
    assert L.flanhip_audio_repitch_plan(100, 48000.0, p(inv), 1, 48, 0, 0, None, None, None, None, None, None, None, None, None) == fa.ERR_INVALID_ARG
    nan = np.full(3, np.nan, np.float32)
    assert L.flanhip_audio_repitch(p(x), 1, 100, 48000.0, p(nan), 3, 48, 0, p(out), None) == fa.ERR_UNSUPPORTED


def test_more_blocks_than_the_cap_are_refused():
    # g = 1 at the upper clamp: about 1000 blocks per input frame, 56 bytes of record each; past 2^22 blocks the loop stops with a refusal
    inv = np.full(5000, 1000.0, np.float32)
    p = inv.ctypes.data_as(ctypes.c_void_p)
    none8 = [None] * 8
    assert fa.lib.flanhip_audio_repitch_plan(5000, 48000.0, p, 5000, 1, 0, 0, *none8, None) == fa.ERR_UNSUPPORTED
    assert "2^22 blocks" in fa.last_error()
    assert fa.lib.flanhip_audio_repitch_plan(4000, 48000.0, p, 5000, 1, 0, 0, *none8, None) > 3900000    # just under the cap: counted


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    c = CASES[IDS.index("up1p5")]
    with pytest.raises(fa.FlanHipError) as e:
        fa.audio_repitch(c["x"], c["sr"], c["inv"], c["g"])
    assert e.value.code == fa.ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------
# the runs of the sinc launch (flanhip_audio_repitch_runs: the launch's own planner, exported)

def planner_shapes():
    """( id, ch, n, sr, inv, g, quality ) of every fixture case, every random seed of the device tests and every run-planner case"""
    shapes = [(c["name"], c["x"].shape[0], c["x"].shape[1], c["sr"], c["inv"], c["g"], c["quality"]) for c in CASES + RUN_CASES]
    for seed in range(20):
        x, sr, inv, g, quality = R.random_case(seed)
        shapes.append(("seed%d" % seed, x.shape[0], x.shape[1], sr, inv, g, quality))
    return shapes


SHAPES = planner_shapes()


def chain(fracpos, ratio, steps):
    """srcpos after `steps` additions of the ratio, as the reference forms it"""
    pos = float(fracpos)
    for _ in range(steps):
        pos += float(ratio)
    return pos


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_runs_tile_the_plan_within_their_limits(shape):
    _, ch, n, sr, inv, g, quality = shape
    p = fa.audio_repitch_plan(n, sr, inv, g, quality)
    r = fa.audio_repitch_runs(n, sr, inv, g, ch, quality)
    blocks = p["offset"].size
    if quality != R.SINC:
        assert r["first_block"].size == 0 and r["channels_per_group"] == 0 and r["groups"] == 0        # the point kernel has no runs
        return
    first, count = r["first_block"], r["num_blocks"].astype(np.int64)
    # every block lies in exactly one run, in order: block b makes output frames [b g, ( b + 1 ) g), so the runs' frames tile [0, blocks g) once
    assert first.size >= 1 and first[0] == 0 and np.all(count >= 1)
    assert np.array_equal(first[1:], first[:-1] + count[:-1]) and first[-1] + count[-1] == blocks
    assert np.array_equal(p["first_out"], np.arange(blocks) * g)
    assert np.all(r["win_len"] >= 0) and np.all(r["win_len"] <= WINDOW_FLOATS)
    assert np.all(count <= max(RUN_OUTPUTS // g, 1))                       # at most 2048 output frames, or one block
    for k in range(first.size):
        a, b = int(first[k]), int(first[k] + count[k])
        for key in ("filtpos", "oversize", "ideal"):
            assert np.all(p[key][a:b] == p[key][a]), (k, key)              # one coefficient table per run
        if r["win_len"][k] > 0:
            lo, hi = int(r["win_start"][k]), int(r["win_start"][k]) + int(r["win_len"][k])
            for blk in range(a, b):                                            # the 64 taps of every block's first and last output are staged
                s_first = int(p["offset"][blk]) + int(p["fracpos"][blk])
                s_last = int(p["offset"][blk]) + int(chain(p["fracpos"][blk], p["ratio"][blk], g - 1))
                assert lo <= s_first and s_last + TAPS <= hi, (k, blk, lo, hi, s_first, s_last)
    cpw, groups = r["channels_per_group"], r["groups"]
    assert cpw >= 1 and groups * cpw >= ch > (groups - 1) * cpw


def test_channel_groups_cover_every_channel_count():
    c = RUN_CASES[RUN_IDS.index("groups_sweep")]
    for ch in range(1, 40):
        r = fa.audio_repitch_runs(c["x"].shape[1], c["sr"], c["inv"], c["g"], ch)
        cpw, groups = r["channels_per_group"], r["groups"]
        assert 1 <= cpw <= ch and groups * cpw >= ch > (groups - 1) * cpw, (ch, cpw, groups)


def test_runs_refusals_and_counting():
    c = RUN_CASES[RUN_IDS.index("window_cut")]
    inv = np.ascontiguousarray(c["inv"])
    p = inv.ctypes.data_as(ctypes.c_void_p)
    L = fa.lib
    n = c["x"].shape[1]
    cpw, groups = ctypes.c_int(-1), ctypes.c_int64(-1)
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, inv.size, c["g"], 0, 2, 0, None, None, None, None, ctypes.byref(cpw), ctypes.byref(groups)) == 2
    assert (cpw.value, groups.value) == (1, 2)
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, inv.size, c["g"], 0, 2, 0, None, None, None, None, None, None) == 2       # everything nullable
    win_len = np.full(1, -1, np.int32)                                         # a capacity below the run count fills that many records
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, inv.size, c["g"], 0, 2, 1, None, None, None, win_len.ctypes.data_as(ctypes.c_void_p), None, None) == 2
    assert 0 < win_len[0] <= WINDOW_FLOATS
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, inv.size, c["g"], 0, 0, 0, None, None, None, None, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch_runs(n, c["sr"], None, inv.size, c["g"], 0, 2, 0, None, None, None, None, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, 1, c["g"], 0, 2, 0, None, None, None, None, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_repitch_runs(n, c["sr"], p, inv.size, c["g"], fa.REPITCH_LINEAR, 2, 0, None, None, None, None, None, None) == fa.ERR_UNSUPPORTED
