"""The loud-chunk scan, Audio::reverse and the methods over them on the MI355X (flan_amd/csrc/temporal.hip, flan_amd/host/Audio.cpp) against
the NumPy restatement (tests/temporal_reference.py): the sequential loop of Audio/AudioTemporal.cpp:20-48 as written, the fades plan in fp32,
the events summed by tests/grains_reference.py's ordered fp32 sum.  Every comparison is exact: chunk tables and summaries are integers, audio
is compared bit for bit.  Workspaces are pre-filled with 0xFF and tables with a sentinel; cases are sized by the kernels' own geometry
(flanhip_loud_run_frames, flanhip_loud_block_frames), read from the library."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch loaded, as in the rest of the suite)

import flan_amd as fa
import grains_reference as G
import host_cpp
import temporal_reference as T

pytestmark = pytest.mark.gpu
F32 = np.float32
SR = 48000.0
SENTINEL = -7
THREADS = fa.loud_block_frames() // fa.loud_run_frames()       # lanes per block
CARRY_PASS = fa.loud_carry_pass_blocks()                       # blocks k_scan_carry takes per pass


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def detect(x, level, gap, run=0, spare=3):
    """( chunks, summary ) through the device entry points, with lanes of `run` frames (0: the library's choice)"""
    x = np.ascontiguousarray(np.atleast_2d(x), F32)
    ch, n = x.shape
    with fa.loud_run_forced(run):
        assert fa.loud_block_frames() == THREADS * fa.loud_run_frames()
        d_x = fa.DeviceArray(host=x)
        d_ws = fa.DeviceArray(host=np.full(fa.loud_workspace_bytes(ch, n), 0xFF, np.uint8))
        d_summary = fa.DeviceArray(host=np.full(4, -1, np.int64))
        fa.loud_summary_dev(d_x, ch, n, level, gap, d_summary, d_ws)
        summary = d_summary.to_host(4, np.int64)
        count = int(summary[0])
        assert 0 <= count <= n
        d_chunks = fa.DeviceArray(host=np.full((count + spare, 2), SENTINEL, np.int32))
        fa.loud_chunks_dev(ch, n, gap, count, d_chunks, count + spare, d_ws)
        chunks = d_chunks.to_host((count + spare, 2), np.int32)
    assert np.all(chunks[count:] == SENTINEL)                   # nothing behind the count
    return chunks[:count].tolist(), summary.tolist()


def check(x, level, gap, run=0):
    x = np.atleast_2d(x)
    got, summary = detect(x, level, gap, run)
    want = T.loud_chunks(x, level, gap)
    assert got == want, (got[:8], want[:8])
    assert summary == T.summary(x, level, gap)
    return got


def spikes(n, frames, ch=1, channel=0):
    x = np.zeros((ch, n), F32)
    x[channel, list(frames)] = 1.0
    return x


# ---- 1. boundaries at the default run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gap", [3, 9])
def test_boundaries_at_the_default_run(gap):
    run, block = fa.loud_run_frames(), fa.loud_block_frames()
    n = 3 * block + 11
    for b in (run, 64 * run, block):                            # a lane's, a wavefront's and a block's first frame
        # noisy at b - 1 and b; the next one gap + 1 later: the same chunk; the one after gap + 2 later: a new chunk.  Then silence to the end:
        # with b = run that is more than a whole block of EMPTY maps through block_scan and the carry
        a = b + gap + 1
        x = spikes(n, [b - 1, b, a, a + gap + 2])
        got = check(x, 0.5, gap)
        assert got == [[b - 1, a], [a + gap + 2, a + gap + 2]]
    # the same pairs straddling the boundaries themselves, a silence of more than one whole block between the first groups, an open end
    frames = []
    for b in (block, 2 * block + 64 * run, 3 * block):
        frames += [b - 1, b + gap]                              # gap + 1 apart across b: one chunk
        if b + 2 * gap + 2 < n - 1:
            frames.append(b + 2 * gap + 2)                      # gap + 2 later: a new one
    x = spikes(n, frames + [n - 1])
    got = check(x, 0.5, gap)
    assert got[:2] == [[block - 1, block + gap], [block + 2 * gap + 2, block + 2 * gap + 2]] and got[-1][1] == n


# ---- 2. the carry's second pass ------------------------------------------------------------------------------------------------------------
def test_carry_second_pass_and_forced_runs():
    n = CARRY_PASS * THREADS + 300                              # run 1: two blocks more than a pass of k_scan_carry takes
    gap = 7
    p = CARRY_PASS * THREADS                                    # run 1: the first frame of the carry's second pass
    # a silence longer than a whole pass of the carry (more than CARRY_PASS blocks at run 1): it crosses the first pass and the pass boundary as
    # EMPTY maps, and the chunk that starts in the second pass must close chunk 0 with end 5.  Then the gap + 1 / gap + 2 pair
    x = spikes(n, [5, p + 40, p + 40 + gap + 1, p + 40 + 2 * gap + 3])
    assert p + 40 - 6 > CARRY_PASS * THREADS
    long_silence = {run: check(x, 0.5, gap, run) for run in (1, 2, 3, 16, 64)}
    assert long_silence[1] == [[5, 5], [p + 40, p + 40 + gap + 1], [p + 40 + 2 * gap + 3, p + 40 + 2 * gap + 3]]
    assert all(t == long_silence[1] for t in long_silence.values())
    # one early chunk, a silence just short of a pass (no single input of this length holds both), then the gap + 1 / gap + 2 pair straddling the
    # pass boundary
    x = spikes(n, [10, 11, p - 1 - (gap + 1), p - 1, p + gap + 1, p + 100, p + 299])
    tables = {run: check(x, 0.5, gap, run) for run in (1, 2, 3, 16, 64)}
    assert tables[1] == [[10, 11], [p - 1 - (gap + 1), p - 1], [p + gap + 1, p + gap + 1], [p + 100, p + 100], [p + 299, n]]
    assert all(t == tables[1] for t in tables.values())
    # the pair the other way round: gap + 2 before the boundary, gap + 1 across it
    x = spikes(n, [p - 2 - (gap + 2), p - 2, p - 2 + gap + 1])
    assert check(x, 0.5, gap, 1) == [[p - 2 - (gap + 2), p - 2 - (gap + 2)], [p - 2, p - 2 + gap + 1]]


# ---- 3. values ---------------------------------------------------------------------------------------------------------------------------
def test_values():
    n = 777
    x = np.zeros((3, n), F32)
    x[2, [100, 101, 300]] = 0.75                                # the only noisy samples are channel 2's
    x[0, 200] = -1.0                                            # a loud negative sample: the compare is signed
    x[1, 400] = np.nan
    assert check(x, 0.5, 10) == [[100, 101], [300, 300]]
    z = np.zeros((2, n), F32)
    z[0, ::2] = -0.0
    assert check(z, 0.0, 3) == []                               # -0.0 and +0.0 are not above 0
    z[1, 5] = np.nan
    z[0, 9] = -3.0
    assert check(z, -1.0, 3) == [[0, n]]                        # a negative level: every frame is noisy, the NaN's and the -3's through the other channel
    w = np.full((1, n), 1.0, F32)
    w[0, 5] = np.nan
    w[0, 9] = -3.0
    assert check(w, -1.0, 0) == [[0, 4], [6, 8], [10, n]]       # mono: the NaN and the -3 are quiet frames


# ---- 4. ends and degenerates ---------------------------------------------------------------------------------------------------------------
def test_ends_and_degenerates():
    n = 1000
    quiet = np.zeros((2, n), F32)
    got, summary = detect(quiet, 0.5, 4)
    assert got == [] and summary == [0, -1, -1, 0]
    assert check(np.ones((2, n), F32), 0.5, 4) == [[0, n]]
    assert check(np.ones((1, 1), F32), 0.5, 4) == [[0, 1]] and check(np.zeros((1, 1), F32), 0.5, 4) == []
    x = spikes(n, [3, 4, 6, 500, 999])
    assert check(x, 0.5, 0) == [[3, 4], [6, 6], [500, 500], [999, n]]
    assert check(x, 0.5, -1) == [[3, 3], [4, 4], [6, 6], [500, 500], [999, 999]]
    assert check(x, 0.5, -2) == check(x, 0.5, -1)
    assert check(x, 0.5, n) == [[3, n]] and check(x, 0.5, 2**31 - 1) == [[3, n]]
    gap = 9
    assert check(spikes(n, [50, n - 2 - gap]), 0.5, gap)[-1] == [n - 2 - gap, n - 2 - gap]      # last + gap + 1 == n - 1: closed by the last frame
    assert check(spikes(n, [50, n - 1 - gap]), 0.5, gap)[-1] == [n - 1 - gap, n]                # last + gap + 1 == n: still open
    with pytest.raises(fa.FlanHipError) as e:                  # a table smaller than the count
        d = fa.DeviceArray(nbytes=64)
        fa.loud_chunks_dev(1, n, gap, 5, d, 4, d)
    assert e.value.code == fa.ERR_INVALID_ARG


# ---- 5. sweep ------------------------------------------------------------------------------------------------------------------------------
def test_sweep_against_the_sequential_loop():
    rng = np.random.default_rng(4242)
    for case in range(200):
        n = int(rng.integers(1, 3001))
        ch = int(rng.integers(1, 4))
        gap = int(rng.integers(-2, 41))
        run = int(rng.integers(1, 4))
        density = float(rng.choice([0.0005, 0.005, 0.05, 0.5]))
        x = np.where(rng.random((ch, n)) < density, rng.uniform(0.5, 1.0, (ch, n)), rng.uniform(-1.0, 0.2, (ch, n))).astype(F32)
        got, summary = detect(x, 0.3, gap, run, spare=1)
        assert got == T.loud_chunks(x, 0.3, gap), (case, n, ch, gap, run)
        assert summary == T.summary(x, 0.3, gap), (case, n, ch, gap, run)


def test_host_form_and_reverse_through_the_c_abi():
    rng = np.random.default_rng(9)
    x = np.where(rng.random((2, 5000)) < 0.01, 1.0, 0.0).astype(F32)
    chunks, summary = fa.loud_chunks(x, 0.5, 20)
    assert chunks.tolist() == T.loud_chunks(x, 0.5, 20) and summary.tolist() == T.summary(x, 0.5, 20)
    for n in (1, 2, 3, 5, 4095, 4096, 4097):
        y = rng.standard_normal((3, n)).astype(F32)
        assert G.same_bits(fa.audio_reverse(y), T.reverse(y)), n


# ---- 6. methods ----------------------------------------------------------------------------------------------------------------------------
BIN, _build, _run = host_cpp.driver("temporal_test")
LEVEL, GAP_TIME = F32(0.2), F32(50.0) / F32(48000.0)
FADES = [0.0, 0.001, 0.05]
FRAMES = 6200                                                  # 2 x 6200 floats also make the 3 x 4097 of the reverse case


def _input():
    """stereo gated noise: channel 0 above the level all through a burst, channel 1 signed.  The first burst starts 20 frames in and the last one
    runs to the end: fades of 0.05 s hit both clamps (AudioTemporal.cpp:58-63); one silence is shorter than the gap"""
    rng = np.random.default_rng(606)
    x = np.zeros((2, FRAMES), F32)
    for lo, hi in ((20, 400), (700, 1500), (1530, 1700), (2500, 2503), (3300, FRAMES)):
        x[0, lo:hi] = rng.uniform(0.4, 1.0, hi - lo)
        x[1, lo:hi] = rng.uniform(-1.0, 1.0, hi - lo)
    return x


@functools.lru_cache(maxsize=None)
def dumped():
    _build()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        _input().tofile(os.path.join(d, "in.f32"))
        _run("--dump", os.path.join(d, "in.f32"), d)
        for name in os.listdir(d):
            if name.endswith(".bin"):
                raw = open(os.path.join(d, name), "rb").read()
                ch, n = np.frombuffer(raw[:8], np.int32)
                out[name[:-4]] = None if n == 0 else np.frombuffer(raw[12:], F32).reshape(int(ch), int(n))
    return out


def _same(name, want):
    got = dumped()[name]
    if want is None or got is None:
        assert want is None and got is None, (name, None if got is None else got.shape, None if want is None else want.shape)
        return
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert G.same_bits(got, want), (name, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:5])


def _same_list(name, wants):
    for i, want in enumerate(wants):
        _same("%s_%d" % (name, i), want)
    assert "%s_%d" % (name, len(wants)) not in dumped()


@pytest.mark.parametrize("k", range(3))
def test_remove_silence_fused_general_and_restatement(k):
    x = _input()
    ev = T.remove_silence_table(x, SR, LEVEL, GAP_TIME, FADES[k])
    assert len(ev) == 4 and np.all(ev["n"] >= 2)
    want = T.render(ev, x, SR)
    _same("rs_fused_%d" % k, want)
    _same("rs_general_%d" % k, want)
    _same_list("chunks_%d" % k, [T.render(t, x, SR) for t in T.chunk_tables(x, SR, LEVEL, GAP_TIME, FADES[k])])
    _same("edge_%d" % k, T.cut_audio(x, SR, *T.edge_cut(x, SR, LEVEL, FADES[k])))


def test_reverse_and_boundaries():
    flat = _input().reshape(-1)
    for n in (1, 2, 4095, 4097):
        _same("reverse_%d" % n, T.reverse(flat[:3 * n].reshape(3, n)))
    x = _input()
    for name, (s, e) in (("mb_pad", (-100, 50)), ("mb_cut", (200, -300)), ("mb_pad_cut", (-37, -41)), ("mb_cut_pad", (64, 10)),
                         ("mb_times", (T.time_to_frame(-0.01, SR), T.time_to_frame(0.02, SR)))):
        _same(name, T.modify_boundaries(x, SR, s, e))


def test_splits():
    x = _input()
    _same_list("split_times", T.split_pieces(x, SR, T.split_frames(FRAMES, SR, [0.05, 0.01, -1.0, 0.08, 9.0]), 0.002))
    _same_list("split_lengths", T.split_pieces(x, SR, T.split_frames(FRAMES, SR, T.split_lengths_times([0.02, -1.0, 0.03, 0.01])), 0.0))
    _same_list("split_equal", T.split_pieces(x, SR, T.split_frames(FRAMES, SR, T.split_lengths_times(T.equal_lengths(FRAMES, SR, 0.03))), 0.001))


def _joined(x, cuts, offsets):
    ev = T._table(cuts, x.shape[1], x.shape[0])
    ev["o"] = T.join_frames([c[1] for c in cuts], offsets, SR)
    return ev


def test_rearrange_and_random_chunks():
    x = _input()
    slice_, fade = F32(0.01), F32(0.002)
    frames = T.split_frames(FRAMES, SR, T.split_lengths_times(T.equal_lengths(FRAMES, SR, F32(slice_ + fade))))
    count = len(frames) - 2
    order = T.rearrange_order(count, 11)
    assert sorted(order) == list(range(count)) and order == fa.rearrange_order(count, 11).tolist()
    ff = T.time_to_frame(fade, SR)
    cuts = [G.cut_frames(FRAMES, frames[p], frames[p + 1], ff, ff) for p in order]
    _same("rearrange", T.render(_joined(x, cuts, [F32(-fade)] * (count + 1)), x, SR))
    cuts, starts, offsets, o = T.random_chunks_plan(FRAMES, SR, 0.1, lambda t: F32(0.005) + F32(0.05) * t, lambda t: F32(0.001) + F32(0.01) * t, 5)
    ev = T._table(cuts, FRAMES, 2)
    ev["o"] = o
    _same("random_chunks", T.render(ev, x, SR))
    # with a mod: every chunk made, scaled by 0.5 + its start time, joined
    plain, grains = G.materialise(ev, x, None, SR)
    at = 0
    for i, c in enumerate(cuts):
        size = 2 * c[1]
        grains[at:at + size] = grains[at:at + size] * F32(F32(0.5) + T.frame_to_time(starts[i], SR))
        at += size
    _same("random_chunks_mod", G.mix32(plain, grains, None, 2, G.out_frames(ev), SR))


def test_iterate_and_delay():
    x = _input()
    _same("iterate", G.mix_method([x] * 3, G.join_times([FRAMES] * 3, [F32(-0.01)] * 4, SR)))
    fed = [(x * F32(0.5)).astype(F32)]
    for _ in range(2):
        fed.append((fed[-1] * F32(0.5)).astype(F32))
    _same("iterate_feedback", G.mix_method(fed, G.join_times([FRAMES] * 3, [F32(-0.0)] * 4, SR)))
    step = F32(1.0) / F32(SR)
    for name, added, delay_time, decay in (("delay_constant", 0.05, lambda t: np.full(t.shape, 0.02, F32), lambda t: np.full(t.shape, 0.5, F32)),
                                           ("delay_ramped", 0.03, lambda t: (F32(0.01) + F32(0.1) * t).astype(F32), lambda t: (F32(0.8) - t).astype(F32))):
        length = F32(F32(FRAMES) / F32(SR)) + F32(added)
        frames = T.time_to_frame(length, SR)
        t = (np.arange(frames).astype(F32) * step).astype(F32)
        sampled_delay, sampled_decay = delay_time(t), decay(t)
        at = (t * F32(SR)).astype(F32).astype(np.int64)        # texture samples the rate at f * step; the rate reads the curve at time_to_frame of that
        rate = np.where(sampled_delay[at] <= 0, F32(1.0) / F32(SR), F32(1.0) / sampled_delay[at]).astype(F32)
        event_frames = G.events(frames, SR, rate)
        times = [G.event_time(f, SR) for f in event_frames]
        chain, fed = x, []
        for i, time in enumerate(times):                       # texture under feedback: event i is event i - 1's result through the mod
            if not (i == 0 or time == 0):                      # the first of a feedback chain is modded at time 0: left alone
                chain = (chain * sampled_decay[T.time_to_frame(time, SR)]).astype(F32)
            fed.append(chain)
        assert len(times) > 3
        _same(name, G.mix_method(fed, times))
