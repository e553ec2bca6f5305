"""Audio::repitch's C ABI (include/flanhip.h, flan_amd/csrc/repitch.hip) without a device: symbols, the host plan against the vectors
the reference's own resampler made, refusals."""
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
SYMBOLS = ["flanhip_audio_repitch_out_frames", "flanhip_audio_repitch_plan", "flanhip_audio_repitch_workspace_bytes",
           "flanhip_audio_repitch", "flanhip_audio_repitch_dev"]
CASES = R.load_cases()
IDS = [c["name"] for c in CASES]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_repitch_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
    for name in ("audio_repitch", "audio_repitch_dev", "audio_repitch_plan", "audio_repitch_out_frames", "audio_repitch_workspace_bytes"):
        assert callable(getattr(fa, name))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name


@pytest.mark.parametrize("case", CASES, ids=IDS)
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
