"""Audio::stereo_spatialize's and pan's C ABI (include/flanhip.h, flan_amd/csrc/spatial.hip) without a device: symbols, the host plan
against the vectors the reference's own resampler made, the workspace layout, refusals."""
import ctypes
import os

import numpy as np
import pytest

import spatial_reference as S


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_spatial_ear", "flanhip_spatial_ear_dev", "flanhip_spatial_delay_dev", "flanhip_spatial_itd_out_frames",
           "flanhip_spatial_itd_plan", "flanhip_spatial_itd_workspace_bytes", "flanhip_spatial_itd", "flanhip_spatial_itd_dev",
           "flanhip_audio_pan", "flanhip_audio_pan_dev", "flanhip_audio_to_stereo_dev", "flanhip_audio_to_mono_dev",
           "flanhip_audio_copy_rows_dev"]
CASES = S.load_cases()
IDS = [c["name"] for c in CASES]
WINDOW_BYTES, BLOCK_BYTES, RUN_BYTES = 64 * 1040 * 8, 56, 64


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_spatial_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
        assert name + "(" in header, name
    for name in ("spatial_ear", "spatial_ear_dev", "spatial_delay_dev", "spatial_itd_out_frames", "spatial_itd_plan", "spatial_itd_workspace_bytes",
                 "spatial_itd", "spatial_itd_dev", "audio_pan", "audio_pan_dev", "audio_to_stereo_dev", "audio_to_mono_dev", "audio_copy_rows_dev"):
        assert callable(getattr(fa, name))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_out_frames_stretches_and_plan_equal_the_references(case):
    n = case["x"].size
    nout, stretches = fa.spatial_itd_out_frames(n, case["sr"], case["dist"])
    assert nout == case["out_frames"]
    assert np.array_equal(stretches, case["stretches"])                     # fp64, the reference's own expression: equal to the bit
    plan = fa.spatial_itd_plan(n, case["sr"], stretches)
    assert plan["delivered"].size == case["blocks"]
    assert np.array_equal(plan["delivered"], case["delivered"])             # what ResampleOut returned, block by block
    assert plan["total_out"] == int(case["delivered"].sum())
    want = S.itd_plan(n, case["sr"], stretches)                             # fp64, the same chain of additions: equal to the bit
    for key, theirs in (("offset", "offset"), ("fracpos", "fracpos"), ("ratio", "ratio"), ("filtpos", "filtpos"), ("oversize", "oversize"),
                        ("first_out", "first_out"), ("delivered", "count"), ("buffered", "buffered")):
        assert np.array_equal(plan[key], np.array([b[theirs] for b in want], plan[key].dtype)), key
    assert np.array_equal(plan["ideal"] != 0, np.array([b["ideal"] for b in want], bool))


def test_plan_of_given_stretches_equals_the_restatement():
    """stretches the method never produces but the C ABI accepts: exact integers and halves (the ideal tables, the GCD branch), the
    ends of the accepted range"""
    for sr, values in ((48000.0, [1.0, 2.0, 0.5, 1.25, 3.0, 0.75, 1.0, 64.0, 0.0625, 1024.0, 1.0, 0.1, 1.0]), (44100.0, [1.0, 0.5, 2.0, 1.5, 1.0])):
        n = 32 * len(values) - 5
        got = fa.spatial_itd_plan(n, sr, np.array(values))
        want = S.itd_plan(n, sr, np.array(values))
        for key, theirs in (("offset", "offset"), ("fracpos", "fracpos"), ("ratio", "ratio"), ("filtpos", "filtpos"), ("oversize", "oversize"),
                            ("first_out", "first_out"), ("delivered", "count"), ("buffered", "buffered")):
            assert np.array_equal(got[key], np.array([b[theirs] for b in want], got[key].dtype)), (sr, key)
        assert np.array_equal(got["ideal"] != 0, np.array([b["ideal"] for b in want], bool))
        assert set(got["oversize"].tolist()) == ({1, 2, 3, 5, 32, 64} if sr == 48000.0 else {1, 2, 3})


def test_plan_counts_without_storage():
    c = CASES[IDS.index("flyby")]
    st = np.ascontiguousarray(c["stretches"])
    total = ctypes.c_int64(0)
    got = fa.lib.flanhip_spatial_itd_plan(4000, c["sr"], p(st), st.size, 0, *([None] * 9), ctypes.byref(total))
    assert got == c["blocks"] and total.value == int(c["delivered"].sum())


def test_workspace_bytes_follow_the_layout():
    """the window factors, 56 bytes per block of every ear, 64 per run"""
    c = CASES[IDS.index("receding")]                                        # one table after the first block: 63 blocks in 2 + 1 runs
    one = fa.spatial_itd_workspace_bytes(2000, c["sr"], c["stretches"])
    runs = (one - WINDOW_BYTES - BLOCK_BYTES * 63) // RUN_BYTES
    assert one == WINDOW_BYTES + BLOCK_BYTES * 63 + RUN_BYTES * runs and 2 <= runs <= 4
    two = fa.spatial_itd_workspace_bytes(2000, c["sr"], np.stack([c["stretches"], c["stretches"]]))
    assert two == WINDOW_BYTES + 2 * (BLOCK_BYTES * 63 + RUN_BYTES * runs)
    a = CASES[IDS.index("approaching")]                                     # a table per block: as many runs as blocks that deliver
    assert fa.spatial_itd_workspace_bytes(2000, a["sr"], a["stretches"]) > WINDOW_BYTES + BLOCK_BYTES * 63 + RUN_BYTES * 40
    j = CASES[IDS.index("jump_away")]                                       # the first block, the second, and a block of 5054 outputs in three runs
    assert fa.spatial_itd_workspace_bytes(80, j["sr"], j["stretches"]) == WINDOW_BYTES + BLOCK_BYTES * 3 + RUN_BYTES * 5
    assert fa.spatial_itd_workspace_bytes(0, c["sr"], c["stretches"]) == 0
    assert fa.spatial_itd_workspace_bytes(2001, c["sr"], c["stretches"][:-1]) == 0          # 63 blocks need 63 stretches


def test_out_frames_refusals():
    d = np.ones(4, np.float64)
    L = fa.lib
    assert L.flanhip_spatial_itd_out_frames(100, 48000.0, None, 4, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_out_frames(100, 48000.0, p(d), 3, None) == fa.ERR_INVALID_ARG          # ceil( 100 / 32 ) = 4
    assert L.flanhip_spatial_itd_out_frames(0, 48000.0, p(d), 4, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_out_frames(100, 0.0, p(d), 4, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_out_frames(100, 48000.0, p(d), 4, None) == 268                          # ceil( ( 128 / 48000 + 1 / 343 ) 48000 )
    assert L.flanhip_spatial_itd_out_frames(32, 48000.0, p(d), 1, None) == 0                             # one block: no output frames


def test_invalid_arguments_are_refused_before_the_device():
    x = np.zeros((2, 100), np.float32)
    st = np.ones((2, 4), np.float64)
    out = np.zeros((2, 300), np.float32)
    nout = np.array([268, 300], np.int64)
    pos = np.zeros((100, 2), np.float64)
    L = fa.lib
    itd = lambda *a: L.flanhip_spatial_itd(*a, None)                        # noqa: E731
    assert itd(p(x), 2, 100, 48000.0, p(st), 4, p(nout), 300, p(out)) in (fa.OK, fa.ERR_NO_DEVICE)
    assert itd(None, 2, 100, 48000.0, p(st), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, 100, 48000.0, None, 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, 100, 48000.0, p(st), 4, None, 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, 100, 48000.0, p(st), 4, p(nout), 300, None) == fa.ERR_INVALID_ARG
    assert itd(p(x), 3, 100, 48000.0, p(st), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG             # one or two ears
    assert itd(p(x), 0, 100, 48000.0, p(st), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, -1, 48000.0, p(st), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, 100, 0.0, p(st), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG
    assert itd(p(x), 2, 100, 48000.0, p(st), 3, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG             # the loop needs 4 stretches
    assert "the loop needs 4" in fa.last_error()
    assert itd(p(x), 2, 100, 48000.0, p(st), 4, p(nout), 299, p(out)) == fa.ERR_INVALID_ARG             # an ear longer than the stride
    for bad in (np.nan, np.inf, -1.0, 0.0, 0.01, 2000.0):
        wrong = st.copy()
        wrong[1, 2] = bad
        assert itd(p(x), 2, 100, 48000.0, p(wrong), 4, p(nout), 300, p(out)) == fa.ERR_INVALID_ARG, bad
        assert "outside [1/16, 1024]" in fa.last_error()
        assert fa.spatial_itd_workspace_bytes(100, 48000.0, wrong) == 0
    ws = ctypes.c_void_p(1 << 40)                                           # never dereferenced: the refusals come first
    assert L.flanhip_spatial_itd_dev(ws, 2, 100, 48000.0, p(st), 4, p(nout), 300, ws, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_dev(None, 2, 100, 48000.0, p(st), 4, p(nout), 300, ws, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_plan(100, 48000.0, p(st), 3, 0, *([None] * 9), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_itd_plan(100, 48000.0, None, 4, 0, *([None] * 9), None) == fa.ERR_INVALID_ARG
    # the ear stage: only mono
    ear = lambda *a: L.flanhip_spatial_ear(*a, None)                        # noqa: E731
    mono = x[0]
    assert ear(p(mono), p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) in (fa.OK, fa.ERR_NO_DEVICE)
    assert ear(p(mono), p(mono), 2, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) == fa.ERR_INVALID_ARG
    assert "mono" in fa.last_error()
    assert ear(None, p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), None, 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, None) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 0, 48000.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 100, -1.0, p(pos), 0.0, 0.0, 0.18, 3, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 0, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, 0.18, 4, p(out)) == fa.ERR_INVALID_ARG
    assert ear(p(mono), p(mono), 1, 100, 48000.0, p(pos), 0.0, 0.0, float("nan"), 3, p(out)) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_ear_dev(ws, ws, 2, 100, 48000.0, ws, 0.0, 0.0, 0.18, 3, ws, None) == fa.ERR_INVALID_ARG
    # the delay, pan, the conversions, the copies
    delays, bad_delays = np.array([3.5, 10.0], np.float32), np.array([3.5, -1.0], np.float32)
    assert L.flanhip_spatial_delay_dev(ws, 2, 100, p(bad_delays), p(nout), 300, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_delay_dev(ws, 2, 100, p(delays), p(nout), 299, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_delay_dev(ws, 3, 100, p(delays), p(nout), 300, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_spatial_delay_dev(None, 2, 100, p(delays), p(nout), 300, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_pan(p(x), 1, 100, None, 0.5, p(out), None) == fa.ERR_INVALID_ARG             # two channels
    assert L.flanhip_audio_pan(p(x), 3, 100, None, 0.5, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_pan(None, 2, 100, None, 0.5, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_pan(p(x), 2, 0, None, 0.5, p(out), None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_pan_dev(ws, 2, 100, None, 0.5, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_to_stereo_dev(None, 100, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_to_stereo_dev(ws, 0, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_to_mono_dev(ws, 0, 100, ws, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_to_mono_dev(ws, 2, 100, None, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_copy_rows_dev(ws, 100, 2, 100, ws, 90, 100, None) == fa.ERR_INVALID_ARG      # a row longer than its stride
    assert L.flanhip_audio_copy_rows_dev(ws, 100, 2, 100, ws, 100, 90, None) == fa.ERR_INVALID_ARG      # the source longer than the destination
    assert L.flanhip_audio_copy_rows_dev(ws, 100, 0, 100, ws, 100, 100, None) == fa.ERR_INVALID_ARG
    assert L.flanhip_audio_copy_rows_dev(None, 100, 2, 100, ws, 100, 100, None) == fa.ERR_INVALID_ARG


def test_more_blocks_than_the_cap_are_refused():
    count = (1 << 22) + 1
    st = np.ones(count, np.float64)
    assert fa.lib.flanhip_spatial_itd_plan(32 * count, 48000.0, p(st), count, 0, *([None] * 9), None) == fa.ERR_UNSUPPORTED
    assert "2^22 blocks" in fa.last_error()
    assert fa.spatial_itd_workspace_bytes(32 * count, 48000.0, st) == 0


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    c = CASES[IDS.index("receding")]
    with pytest.raises(fa.FlanHipError) as e:
        fa.spatial_itd(c["x"], c["sr"], c["stretches"], c["out_frames"])
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.spatial_ear(c["x"], c["x"], c["sr"], (1.0, 1.0))
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.audio_pan(np.zeros((2, 10), np.float32), 0.5)
    assert e.value.code == fa.ERR_NO_DEVICE
