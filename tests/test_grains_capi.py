"""The C ABI of Audio::mix and the granular family (include/flanhip.h, flan_amd/csrc/grains.hip) without a device: symbols, the host-only
functions bit for bit against the restatement (tests/grains_reference.py), refusals, FLANHIP_ERR_NO_DEVICE."""
import ctypes
import os

import numpy as np
import pytest

import grains_reference as R


class _LazyLib:
    """flan_amd, imported at first use: the HIP runtime is initialised after torch's (as the other GPU test modules do it)"""

    def __getattr__(self, name):
        import flan_amd
        return getattr(flan_amd, name)


fa = _LazyLib()

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["flanhip_grains_tile_frames", "flanhip_grains_batch_events", "flanhip_grains_events", "flanhip_grains_cut", "flanhip_grains_cut_frames",
           "flanhip_grains_plan", "flanhip_grains_workspace_bytes", "flanhip_grains_mix_dev", "flanhip_grains_mix"]


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def test_symbols_are_exported_and_bound():
    lib = ctypes.CDLL(os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    header = open(os.path.join(ROOT, "include", "flanhip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in fa.EXPORTS, name
        assert name + "(" in header, name
    for name in ("grains_events", "grains_cut", "grains_cut_frames", "grains_plan", "grains_workspace_bytes", "grains_mix_dev", "grains_mix",
                 "grains_tile_frames", "grains_batch_events"):
        assert callable(getattr(fa, name))
    for cited in ("AudioCombination.cpp:102-170", "AudioSynthesis.cpp:310-374", "AudioTemporal.cpp:207-234", "AudioVolume.cpp:111-118",
                  "WindowFunctions.cpp:10-13", ":146-150", "AudioSynthesis.cpp:626"):
        assert cited in header, cited
    assert "grains.hip" in open(os.path.join(ROOT, "flan_amd", "build.py")).read()
    assert fa.GRAIN_EVENT == R.EVENT and fa.GRAIN_EVENT.itemsize == 72 and fa.GRAIN_HANN == R.HANN
    assert fa.grains_tile_frames() > 0 and fa.grains_batch_events() > 0


def test_events_are_the_restatement_s():
    rng = np.random.default_rng(11)
    cases = [(1000, 48000.0, 0.0), (1000, 48000.0, -3.0), (20, 48000.0, 12000.0), (5, 48000.0, 3 * 48000.0), (4801, 48000.0, 2000.0), (4410, 44100.0, 777.7),
             (3000, 48000.0, rng.uniform(-500, 5000, 3000).astype(F32)), (3000, 22050.0, (2000 * np.sin(np.arange(3000) / 200.0) ** 2).astype(F32))]
    for length, sr, rate in cases:
        got = fa.grains_events(length, sr, rate)
        assert got.dtype == np.int64 and np.array_equal(got, R.events(length, sr, rate)), (length, sr)
        assert got[0] == 0                                                      # the accumulator starts at 1
    assert np.array_equal(fa.grains_events(1000, 48000.0, 0.0), [0])            # a rate of 0: that event alone
    # scatter 0 draws nothing: the seed does not matter; a scatter curve of zeros neither
    assert np.array_equal(fa.grains_events(4801, 48000.0, 2000.0, 0.0, 1), fa.grains_events(4801, 48000.0, 2000.0, np.zeros(4801, F32), 99))
    assert np.array_equal(fa.grains_events(4801, 48000.0, 2000.0, -1.0, 5), R.events(4801, 48000.0, 2000.0))      # the scatter is clamped at 0


def test_scattered_events_are_sorted_inside_and_repeatable():
    length, sr = 9600, 48000.0
    plain = fa.grains_events(length, sr, 2000.0)
    moved = 0
    for seed in (1, 2, 12345):
        for scatter in (0.5, 40.0, np.linspace(0, 30, length).astype(F32)):
            got = fa.grains_events(length, sr, 2000.0, scatter, seed)
            assert np.all(np.diff(got) >= 0) and got.size > 0 and got[0] >= 0 and got[-1] < length
            assert got.size <= plain.size
            assert np.array_equal(got, fa.grains_events(length, sr, 2000.0, scatter, seed))
            moved += not np.array_equal(got, plain)
    assert moved == 9
    assert fa.grains_events(length, sr, 2000.0, 40.0, 1).size < plain.size      # sigma = 960 frames: some leave [0, length)
    assert not np.array_equal(fa.grains_events(length, sr, 2000.0, 0.5, 1), fa.grains_events(length, sr, 2000.0, 0.5, 2))
    # sigma = scatter / rate * sr: 0.5 / 2000 * 48000 = 12 frames
    d = fa.grains_events(length, sr, 2000.0, 0.5, 7)
    assert d.size > 0.95 * plain.size


def test_cut_is_the_restatement_s():
    rng = np.random.default_rng(5)
    N, sr = 5000, 48000.0
    count = 400
    start = rng.uniform(-0.02, 0.12, count).astype(F32)
    length = rng.uniform(-0.01, 0.05, count).astype(F32)
    fade = rng.uniform(-0.005, 0.04, count).astype(F32)
    fade2 = rng.uniform(-0.005, 0.04, count).astype(F32)
    with np.errstate(all="ignore"):
        length[:6] = [np.inf, -np.inf, np.nan, 1e30, F32(2.0) / F32(0.0), 0.0]   # the non-finite grain lengths
        start[6:8] = [np.nan, np.inf]
        fade[8:10] = [np.nan, np.inf]
        end = (start + length).astype(F32)
    got = fa.grains_cut(N, sr, start, end, fade, fade2)
    want = R.cut_table(N, sr, start, end, fade, fade2)
    for field in ("s", "n", "sf", "ef"):
        assert np.array_equal(got[field], want[field]), field
    assert np.all(got["n"][:10] == 0)
    assert np.all(got["sf"] + got["ef"] <= got["n"]) and np.all(got["s"] + got["n"] <= N - 1 + (got["n"] == 0))
    assert 50 < np.count_nonzero(got["n"] == 0) < 300 and np.any((got["n"] > 0) & (got["sf"] + got["ef"] > got["n"] - 3))      # the rescale is exercised
    # the other fields are left alone
    e = R.make_events(3)
    e["o"], e["gain"] = [5, 6, 7], 0.25
    fa.grains_cut(N, sr, [0.0, 0.01, 0.02], [0.01, 0.03, 0.02], [0.0] * 3, [0.0] * 3, e)
    assert list(e["o"]) == [5, 6, 7] and np.all(e["gain"] == F32(0.25)) and list(e["n"]) == [480, 960, 0]
    # frames
    by_hand = [(10, 10, 0, 0), (20, 10, 0, 0), (200, 300, 0, 0), (-50, -10, 0, 0), (-5, 10, 0, 0), (90, 500, 0, 0), (98, 99, 3, 3), (0, 10, 8, 8),
               (0, 6, 7, 2), (0, 10, -3, 4), (0, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)]
    a = np.array(by_hand, np.int32)
    got = fa.grains_cut_frames(100, a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    for k, row in enumerate(by_hand):
        assert (got["s"][k], got["n"][k], got["sf"][k], got["ef"][k]) == R.cut_frames(100, *row), row


def test_plan_is_the_restatement_s():
    tile = fa.grains_tile_frames()
    rng = np.random.default_rng(8)
    for count in (0, 1, 7, 300):
        e = R.make_events(count)
        e["channels"], e["src_frames"], e["ch_stride"] = 1, 10 * tile, 10 * tile
        e["n"] = rng.integers(0, 3 * tile, count)
        e["n"][rng.random(count) < 0.2] = 0
        e["o"] = rng.integers(-2 * tile, 9 * tile, count)
        if count > 2:
            e["o"][1], e["n"][1] = 2 * tile, tile                             # from a tile's first frame to its last
        frames, first, last = fa.grains_plan(e)
        want = R.plan(e, tile)
        assert frames == want[0] and np.array_equal(first, want[1]) and np.array_equal(last, want[2]), count
    e = R.make_events(2)
    e["o"], e["n"] = [3 * tile + 5, 0], [0, 0]
    assert fa.grains_plan(e)[0] == 3 * tile + 5                                 # an empty event counts for the length


def test_invalid_arguments_are_refused_before_the_device():
    L = fa.lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    dev = [ctypes.c_void_p((1 << 40) + (k << 30)) for k in range(4)]     # never dereferenced: the refusals come first
    tile = fa.grains_tile_frames()

    def refused(rc, words, code=None):
        assert rc == (fa.ERR_INVALID_ARG if code is None else code), (rc, fa.last_error())
        assert words in fa.last_error(), fa.last_error()

    def table():
        e = R.make_events(2)
        e["ch_stride"], e["src_frames"], e["channels"], e["n"], e["o"] = 1000, 1000, 2, 500, [0, 700]
        return e

    def mix_dev(e, first=None, last=None, tiles=None, gains=dev[0], gain_floats=2000, sources=dev[1], sources_floats=2000, channels=2, frames=1200,
                sr=48000.0, out=dev[2], ws=dev[3], count=None):
        f = np.zeros(2, np.int32) if first is None else first
        la = np.ones(2, np.int32) if last is None else last
        return L.flanhip_grains_mix_dev(None if e is None else p(e), (0 if e is None else e.size) if count is None else count,
                                        None if first is False else p(f), None if last is False else p(la), 2 if tiles is None else tiles,
                                        gains, gain_floats, sources, sources_floats, channels, frames, sr, out, ws, None)

    assert 1200 > tile and 1200 <= 2 * tile
    refused(mix_dev(table(), out=None), "null buffer")
    refused(mix_dev(table(), ws=None), "null workspace")
    refused(mix_dev(table(), first=False), "null plan")
    refused(mix_dev(table(), last=False), "null plan")
    refused(mix_dev(None, count=2), "null event table")
    refused(mix_dev(table(), count=-1), "event count out of range")
    refused(mix_dev(table(), channels=0), "non-positive size")
    refused(mix_dev(table(), frames=0), "non-positive size")
    refused(mix_dev(table(), frames=-5), "non-positive size")
    refused(mix_dev(table(), sr=0.0), "sample_rate <= 0")
    refused(mix_dev(table(), sr=-48000.0), "sample_rate <= 0")
    refused(mix_dev(table(), gain_floats=-1), "negative size")
    refused(mix_dev(table(), tiles=3), "num_tiles is not the output's tile count")
    refused(mix_dev(table(), last=np.array([1, 2], np.int32)), "the plan names events the table does not hold")
    refused(mix_dev(table(), first=np.array([-1, 0], np.int32)), "the plan names events the table does not hold")
    for field, value, words in (("s", -1, "source range leaves its buffer"), ("s", 501, "source range leaves its buffer"),
                                ("src_frames", 400, "source range leaves its buffer"), ("src", 600, "source range leaves its buffer"),
                                ("ch_stride", 1600, "source range leaves its buffer"), ("ch_stride", -1, "source range leaves its buffer"),
                                ("n", -4, "negative size"), ("channels", -1, "negative size"), ("flags", 2, "unknown flags"),
                                ("sf", 300, "fades are longer"), ("ef", -1, "fades are longer"), ("gain_offset", 1501, "gains leave the pool"),
                                ("o", 1 << 61, "output frame out of range")):
        e = table()
        if field in ("sf",):
            e["ef"][1] = 201
        e[field][1] = value
        refused(mix_dev(e), words)
    e = table()
    e["gain_offset"][0] = 0
    refused(mix_dev(e, gains=None), "gains leave the pool")
    e = table()
    e["src"][1] = 0
    refused(mix_dev(e, sources=None), "null source")
    # the host form
    src, out = np.zeros(2000, F32), np.zeros((2, 1200), F32)

    def mix(e, sources=src, channels=2, frames=1200, sr=48000.0, out_=out):
        return L.flanhip_grains_mix(p(e), e.size, None, 0, None if sources is None else p(sources), 0 if sources is None else sources.size, channels,
                                    frames, sr, None if out_ is None else p(out_), None)

    refused(mix(table(), out_=None), "null buffer")
    refused(mix(table(), sources=None), "null buffer")
    refused(mix(table(), channels=0), "non-positive size")
    refused(mix(table(), sr=0.0), "sample_rate <= 0")
    e = table()
    e["s"][0] = 501
    refused(mix(e), "source range leaves its buffer")
    # the host-only functions
    n = ctypes.c_int64(0)
    np_ = ctypes.cast(ctypes.byref(n), ctypes.c_void_p)
    frames = np.zeros(100, np.int64)
    refused(L.flanhip_grains_events(100, 48000.0, None, 10.0, None, 0.0, 0, p(frames), 100, None), "null buffer")
    refused(L.flanhip_grains_events(0, 48000.0, None, 10.0, None, 0.0, 0, p(frames), 100, np_), "non-positive size")
    refused(L.flanhip_grains_events(100, 0.0, None, 10.0, None, 0.0, 0, p(frames), 100, np_), "sample_rate <= 0")
    refused(L.flanhip_grains_events(100, 48000.0, None, 10.0, None, 0.0, 0, None, 100, np_), "null buffer")
    refused(L.flanhip_grains_events(100, 48000.0, None, 48000.0, None, 0.0, 0, p(frames), 50, np_), "too small")
    assert L.flanhip_grains_events(100, 48000.0, None, 48000.0, None, 0.0, 0, None, 0, np_) == fa.OK and n.value == 100      # the count alone
    t = np.zeros(2, F32)
    refused(L.flanhip_grains_cut(0, 48000.0, 2, p(t), p(t), p(t), p(t), p(table())), "non-positive size")
    refused(L.flanhip_grains_cut(100, 0.0, 2, p(t), p(t), p(t), p(t), p(table())), "sample_rate <= 0")
    refused(L.flanhip_grains_cut(100, 48000.0, 2, None, p(t), p(t), p(t), p(table())), "null buffer")
    refused(L.flanhip_grains_cut(100, 48000.0, 2, p(t), p(t), p(t), p(t), None), "null buffer")
    refused(L.flanhip_grains_cut_frames(100, 2, None, p(t), p(t), p(t), p(table())), "null buffer")
    refused(L.flanhip_grains_cut_frames(-1, 2, p(t), p(t), p(t), p(t), p(table())), "non-positive size")
    n.value = 0                                                           # in: 0 asks for the reference's length
    refused(L.flanhip_grains_plan(p(table()), 2, None, None, None, 0), "null buffer")
    refused(L.flanhip_grains_plan(None, 2, np_, None, None, 0), "null event table")
    one = np.zeros(1, np.int32)
    refused(L.flanhip_grains_plan(p(table()), 2, np_, p(one), None, 2), "null buffer")
    refused(L.flanhip_grains_plan(p(table()), 2, np_, p(one), p(one), 1), "num_tiles is not the output's tile count")
    assert n.value == 1200
    assert fa.grains_plan(table(), 700)[0] == 700 and fa.grains_plan(table(), 700)[1].size == 1      # the caller's own length
    assert fa.grains_workspace_bytes(-1, 100) == 0 and fa.grains_workspace_bytes(5, 0) == 0
    assert fa.grains_workspace_bytes(0, 1) > 0 and fa.grains_workspace_bytes(1000, 10 * tile) >= 1000 * 72 + 2 * 4 * 10


def test_a_valid_call_without_a_device_says_so():
    if not _no_gpu():
        pytest.skip("a GPU is visible here; the no-device answer is checked in the CPU container")
    e = R.make_events(1)
    e["ch_stride"], e["src_frames"], e["channels"], e["n"] = 100, 100, 1, 100
    with pytest.raises(fa.FlanHipError) as err:
        fa.grains_mix(e, None, np.zeros(100, F32), 1, 100, 48000.0)
    assert err.value.code == fa.ERR_NO_DEVICE
    dev = [ctypes.c_void_p((1 << 40) + (k << 30)) for k in range(3)]
    frames, first, last = fa.grains_plan(e)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                      # noqa: E731
    assert fa.lib.flanhip_grains_mix_dev(p(e), 1, p(first), p(last), first.size, None, 0, dev[0], 100, 1, frames, 48000.0, dev[1], dev[2], None) == fa.ERR_NO_DEVICE
