"""The host-only entry points of the silence-removal and slicing family (include/flanhip.h, flan_amd/csrc/temporal.hip) against the NumPy
restatement (tests/temporal_reference.py) over seeded random arguments -- all integers and fp32 values, compared exactly --, every refusal, and
FLANHIP_ERR_NO_DEVICE from the compute entry points when no GPU is visible.  No compute here."""
import ctypes as C

import numpy as np
import pytest

import flan_amd as fa
import temporal_reference as T

F32 = np.float32
lib = fa.lib
_vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(_vp)


def _random_chunks(rng, n):
    """an ascending chunk table inside [0, n], the last chunk open now and then"""
    count = int(rng.integers(1, 9))
    marks = np.sort(rng.choice(np.arange(0, n), size=min(2 * count, n), replace=False))
    chunks = [[int(marks[2 * i]), int(marks[2 * i + 1])] for i in range(len(marks) // 2)]
    if not chunks:
        chunks = [[0, 0]]
    if rng.random() < 0.4:
        chunks[-1][1] = n
    return chunks


def test_fades_plan_is_the_restatement_s():
    rng = np.random.default_rng(11)
    for case in range(300):
        n = int(rng.integers(2, 5000))
        sr = float(rng.choice([1000.0, 44100.0, 48000.0]))
        chunks = _random_chunks(rng, n)
        fade = float(F32(rng.choice([0.0, 0.0005, 0.003, 0.02, 0.5, -0.001])))
        cuts, _, offsets = T.fades(n, sr, chunks, fade)
        ev, off = fa.loud_chunks_fades(n, sr, chunks, fade, join=True)
        assert [(int(e["s"]), int(e["n"]), int(e["sf"]), int(e["ef"])) for e in ev] == cuts, (case, chunks, fade)
        assert off.view(np.uint32).tolist() == np.array(offsets, F32).view(np.uint32).tolist(), case
        assert ev["o"].tolist() == T.join_frames([c[1] for c in cuts], offsets, sr), case
        plain, _ = fa.loud_chunks_fades(n, sr, chunks, fade, join=False)
        assert np.all(plain["o"] == 0) and plain["n"].tolist() == ev["n"].tolist()


def test_edge_cut_split_frames_and_order_are_the_restatement_s():
    rng = np.random.default_rng(12)
    for case in range(300):
        n = int(rng.integers(1, 5000))
        sr = float(rng.choice([1000.0, 44100.0, 48000.0]))
        x = np.zeros((1, n), F32)
        if rng.random() < 0.9:
            x[0, rng.integers(0, n, int(rng.integers(1, 4)))] = 1.0
        fade = float(F32(rng.choice([0.0, 0.001, 0.01, 0.3])))
        summary = T.summary(x, 0.5, 0)
        assert fa.edge_silence_cut(n, sr, summary[1], summary[2], fade) == T.edge_cut(x, sr, 0.5, fade), case
        times = (rng.uniform(-0.1, 1.5 * n / sr, int(rng.integers(0, 12)))).astype(F32)
        assert fa.split_frames(n, sr, times).tolist() == T.split_frames(n, sr, times), case
        count = int(rng.integers(1, 40))
        seed = int(rng.integers(0, 2**32))
        order = fa.rearrange_order(count, seed).tolist()
        assert order == T.rearrange_order(count, seed) and sorted(order) == list(range(count)), case
    assert fa.split_frames(100, 1000.0, [np.inf, 0.05, -np.inf]).tolist() == [0, 50, 100]


def test_random_chunks_plan_is_the_restatement_s():
    rng = np.random.default_rng(13)
    for case in range(40):
        n = int(rng.integers(100, 20000))
        sr = float(rng.choice([1024.0, 44100.0, 48000.0]))
        length = float(F32(rng.uniform(0.01, 0.2)))
        seed = int(rng.integers(0, 2**32))
        frames = fa.random_chunks_frames(sr, length)
        assert frames == T.random_chunks_loop_frames(sr, length)
        if case % 2:
            cl, fd = float(F32(rng.uniform(0.0, 0.05))), float(F32(rng.uniform(0.0, 0.01)))
            want = T.random_chunks_plan(n, sr, length, cl, fd, seed)
            ev, starts, offsets = fa.random_chunks_plan(n, sr, length, cl, fd, seed)
        else:
            a, b = F32(rng.uniform(0.001, 0.02)), F32(rng.uniform(0.0, 0.3))
            c, d = F32(rng.uniform(0.0, 0.005)), F32(rng.uniform(0.0, 0.05))
            t = (np.arange(frames + 1).astype(F32) / F32(sr)).astype(F32)
            want = T.random_chunks_plan(n, sr, length, lambda s: F32(a + b * s), lambda s: F32(c + d * s), seed)
            ev, starts, offsets = fa.random_chunks_plan(n, sr, length, (a + b * t[:frames]).astype(F32), (c + d * t).astype(F32), seed)
        cuts, want_starts, want_offsets, want_o = want
        assert [(int(e["s"]), int(e["n"]), int(e["sf"]), int(e["ef"])) for e in ev] == cuts, case
        assert starts.tolist() == want_starts and ev["o"].tolist() == want_o, case
        assert offsets.view(np.uint32).tolist() == np.array(want_offsets, F32).view(np.uint32).tolist(), case


def _refused(rc):
    assert rc == fa.ERR_INVALID_ARG, rc
    assert fa.last_error()


def test_refusals_before_any_device_call():
    ev = np.zeros(4, fa.GRAIN_EVENT)
    chunks = np.array([[1, 2], [5, 9]], np.int32)
    off = np.zeros(5, F32)
    i64 = C.c_int64(0)
    pc = C.cast(C.byref(i64), _vp)
    big = 2**31
    # the fades plan
    _refused(lib.flanhip_loud_chunks_fades(100, 48000.0, None, 2, 0.0, 0, _p(ev), _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(100, 48000.0, _p(chunks), 2, 0.0, 0, None, _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(0, 48000.0, _p(chunks), 2, 0.0, 0, _p(ev), _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(100, 48000.0, _p(chunks), 0, 0.0, 0, _p(ev), _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(big, 48000.0, _p(chunks), 2, 0.0, 0, _p(ev), _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(100, 0.0, _p(chunks), 2, 0.0, 0, _p(ev), _p(off)))
    _refused(lib.flanhip_loud_chunks_fades(100, 48000.0, _p(chunks), big, 0.0, 0, _p(ev), _p(off)))          # longer than the mix takes
    _refused(lib.flanhip_loud_chunks_fades(8, 48000.0, _p(chunks), 2, 0.0, 0, _p(ev), _p(off)))              # a chunk outside the frames
    _refused(lib.flanhip_loud_chunks_fades(100, 48000.0, _p(chunks), 2, float("inf"), 0, _p(ev), _p(off)))
    assert lib.flanhip_loud_chunks_fades(100, 48000.0, _p(chunks), 2, 0.0, 0, _p(ev), None) == fa.OK          # the offsets are optional
    # the edge cut
    out4 = np.zeros(4, np.int32)
    _refused(lib.flanhip_edge_silence_cut(100, 48000.0, 1, 5, 0.0, None))
    _refused(lib.flanhip_edge_silence_cut(0, 48000.0, -1, -1, 0.0, _p(out4)))
    _refused(lib.flanhip_edge_silence_cut(big, 48000.0, 1, 5, 0.0, _p(out4)))
    _refused(lib.flanhip_edge_silence_cut(100, -1.0, 1, 5, 0.0, _p(out4)))
    _refused(lib.flanhip_edge_silence_cut(100, 48000.0, 5, 1, 0.0, _p(out4)))
    _refused(lib.flanhip_edge_silence_cut(100, 48000.0, 5, 100, 0.0, _p(out4)))
    _refused(lib.flanhip_edge_silence_cut(100, 48000.0, 1, 5, float("nan"), _p(out4)))
    # the splits
    times = np.array([0.1, 0.2], F32)
    frames = np.zeros(4, np.int32)
    _refused(lib.flanhip_split_frames(100, 48000.0, _p(times), 2, _p(frames), 4, None))
    _refused(lib.flanhip_split_frames(100, 48000.0, None, 2, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(100, 48000.0, _p(times), 2, None, 4, pc))
    _refused(lib.flanhip_split_frames(0, 48000.0, _p(times), 2, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(big, 48000.0, _p(times), 2, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(100, 0.0, _p(times), 2, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(100, 48000.0, _p(times), -1, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(100, 48000.0, _p(times), big, _p(frames), 4, pc))
    _refused(lib.flanhip_split_frames(100000, 48000.0, _p(times), 2, _p(frames), 3, pc))                     # four frames do not fit three
    _refused(lib.flanhip_split_frames(100, 48000.0, _p(np.array([0.1, np.nan], F32)), 2, _p(frames), 4, pc))
    assert lib.flanhip_split_frames(100000, 48000.0, _p(times), 2, None, 0, pc) == fa.OK and i64.value == 4  # the count alone
    # the order
    _refused(lib.flanhip_rearrange_order(3, 1, None))
    _refused(lib.flanhip_rearrange_order(0, 1, _p(frames)))
    _refused(lib.flanhip_rearrange_order(big, 1, _p(frames)))
    # random_chunks
    starts = np.zeros(4, np.int32)
    assert lib.flanhip_random_chunks_frames(0.0, 1.0) == -1 and lib.flanhip_random_chunks_frames(48000.0, 0.0) == -1
    assert lib.flanhip_random_chunks_frames(48000.0, float("nan")) == -1 and lib.flanhip_random_chunks_frames(48000.0, 1e9) == -1
    args = (None, 0.01, None, 0.0, 1)
    _refused(lib.flanhip_random_chunks_plan(100, 48000.0, 0.01, *args, _p(ev), _p(starts), _p(off), 4, None))
    _refused(lib.flanhip_random_chunks_plan(0, 48000.0, 0.01, *args, _p(ev), _p(starts), _p(off), 4, pc))
    _refused(lib.flanhip_random_chunks_plan(big, 48000.0, 0.01, *args, _p(ev), _p(starts), _p(off), 4, pc))
    _refused(lib.flanhip_random_chunks_plan(100, 0.0, 0.01, *args, _p(ev), _p(starts), _p(off), 4, pc))
    _refused(lib.flanhip_random_chunks_plan(100, 48000.0, 0.0, *args, _p(ev), _p(starts), _p(off), 4, pc))
    _refused(lib.flanhip_random_chunks_plan(100, 48000.0, 0.01, *args, None, _p(starts), _p(off), 4, pc))
    _refused(lib.flanhip_random_chunks_plan(10000, 48000.0, 0.1, None, 0.001, None, 0.0, 1, _p(ev), _p(starts), _p(off), 4, pc))      # 100 chunks do not fit 4
    # the device entry points check their arguments before they look for a device
    bogus = _vp(1 << 41)
    assert lib.flanhip_loud_workspace_bytes(0, 100) == 0 and lib.flanhip_loud_workspace_bytes(2, 0) == 0 and lib.flanhip_loud_workspace_bytes(2, big) == 0
    assert lib.flanhip_loud_workspace_bytes(2, 100000) > 0
    _refused(lib.flanhip_loud_summary_dev(None, 2, 100, 0.5, 4, bogus, bogus, None))
    _refused(lib.flanhip_loud_summary_dev(bogus, 2, 100, 0.5, 4, None, bogus, None))
    _refused(lib.flanhip_loud_summary_dev(bogus, 2, 100, 0.5, 4, bogus, None, None))
    _refused(lib.flanhip_loud_summary_dev(bogus, 0, 100, 0.5, 4, bogus, bogus, None))
    _refused(lib.flanhip_loud_summary_dev(bogus, 2, 0, 0.5, 4, bogus, bogus, None))
    _refused(lib.flanhip_loud_summary_dev(bogus, 2, big, 0.5, 4, bogus, bogus, None))
    _refused(lib.flanhip_loud_chunks_dev(2, 100, 4, 3, None, 3, bogus, None))
    _refused(lib.flanhip_loud_chunks_dev(2, 100, 4, 3, bogus, 3, None, None))
    _refused(lib.flanhip_loud_chunks_dev(2, 100, 4, 3, bogus, 2, bogus, None))                              # a capacity below the count
    _refused(lib.flanhip_loud_chunks_dev(2, 100, 4, -1, bogus, 3, bogus, None))
    _refused(lib.flanhip_loud_chunks_dev(2, big, 4, 3, bogus, 3, bogus, None))
    _refused(lib.flanhip_loud_chunks_dev(0, 100, 4, 3, bogus, 3, bogus, None))
    x = np.zeros((2, 100), F32)
    summary = np.zeros(4, np.int64)
    _refused(lib.flanhip_loud_chunks(None, 2, 100, 0.5, 4, None, 0, _p(summary), None))
    _refused(lib.flanhip_loud_chunks(_p(x), 2, 100, 0.5, 4, None, 0, None, None))
    _refused(lib.flanhip_loud_chunks(_p(x), 2, 100, 0.5, 4, None, 3, _p(summary), None))
    _refused(lib.flanhip_loud_chunks(_p(x), 2, 0, 0.5, 4, None, 0, _p(summary), None))
    _refused(lib.flanhip_loud_chunks(_p(x), 2, big, 0.5, 4, None, 0, _p(summary), None))
    _refused(lib.flanhip_audio_reverse_dev(None, 2, 100, bogus, None))
    _refused(lib.flanhip_audio_reverse_dev(bogus, 2, 100, None, None))
    _refused(lib.flanhip_audio_reverse_dev(bogus, 2, 100, bogus, None))                                     # the output is the input
    _refused(lib.flanhip_audio_reverse_dev(bogus, 2, 100, _vp((1 << 41) + 796), None))                      # its first float is the input's last
    _refused(lib.flanhip_audio_reverse_dev(_vp((1 << 41) + 400), 2, 100, bogus, None))                      # overlapping from the other side
    _refused(lib.flanhip_audio_reverse_dev(bogus, 0, 100, _vp(1 << 42), None))
    _refused(lib.flanhip_audio_reverse_dev(bogus, 2, big, _vp(1 << 42), None))
    _refused(lib.flanhip_audio_reverse(_p(x), 2, 100, None, None))
    _refused(lib.flanhip_audio_reverse(_p(x), 2, 0, _p(x), None))


def test_debug_run_and_geometry():
    assert fa.loud_run_frames() >= 1 and fa.loud_block_frames() % fa.loud_run_frames() == 0 and fa.loud_carry_pass_blocks() >= 1
    default = fa.loud_workspace_bytes(2, 100000)
    with fa.loud_run_forced(1):
        assert fa.loud_run_frames() == 1 and fa.loud_block_frames() == fa.loud_carry_pass_blocks()      # both are the block's threads
        assert fa.loud_workspace_bytes(2, 100000) > default     # a mask per lane: more lanes, more masks
    with fa.loud_run_forced(1000):
        assert fa.loud_run_frames() == 64                       # a mask holds 64 frames
    assert fa.loud_workspace_bytes(2, 100000) == default


def test_no_device_is_loud():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible here; the no-device behaviour is checked in the CPU container")
    x = np.zeros((2, 1000), F32)
    with pytest.raises(fa.FlanHipError) as e:
        fa.loud_chunks(x, 0.5, 10)
    assert e.value.code == fa.ERR_NO_DEVICE
    with pytest.raises(fa.FlanHipError) as e:
        fa.audio_reverse(x)
    assert e.value.code == fa.ERR_NO_DEVICE
    for call in (lambda: fa.loud_summary_dev(1 << 41, 2, 1000, 0.5, 10, 1 << 42, 1 << 43),
                 lambda: fa.loud_chunks_dev(2, 1000, 10, 3, 1 << 41, 3, 1 << 43),
                 lambda: fa.audio_reverse_dev(1 << 41, 2, 1000, 1 << 42)):
        with pytest.raises(fa.FlanHipError) as e:
            call()
        assert e.value.code == fa.ERR_NO_DEVICE
