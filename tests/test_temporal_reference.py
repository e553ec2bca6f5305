"""tests/temporal_reference.py, the NumPy restatement of Audio/AudioTemporal.cpp's silence removal and slicing, against cases worked by hand from
the reference's text: what the GPU suite compares the device with must itself say what the reference says."""
import numpy as np

import grains_reference as G
import temporal_reference as T

F32 = np.float32
SR = 48000.0


def _spikes(n, frames, value=1.0):
    x = np.zeros((1, n), F32)
    x[0, list(frames)] = value
    return x


def test_a_chunk_ends_at_its_last_noisy_frame_and_an_open_one_at_num_frames():
    # gap 2: frames 3 and 5 are one chunk (at frame 4, 4 - 3 = 1 is not above 2); frame 8 closes it (8 - 5 = 3) with end 5, the LAST NOISY frame,
    # not 8.  Frame 17 opens a chunk that frame 19, the last, does not close (19 - 17 = 2): it is pushed with end num_frames = 20
    x = _spikes(20, [3, 5, 17])
    assert T.loud_chunks(x, 0.5, 2) == [[3, 5], [17, 20]]
    assert T.loud_chunks(_spikes(21, [3, 5, 17]), 0.5, 2) == [[3, 5], [17, 17]]      # one frame more and it is closed: 20 - 17 = 3
    assert T.loud_chunks(x, 0.5, -1) == [[3, 3], [5, 5], [17, 17]]                  # a negative gap: every noisy frame its own chunk
    assert T.loud_chunks(np.zeros((2, 9), F32), 0.5, 2) == []
    assert T.summary(x, 0.5, 2) == [2, 3, 17, 0] and T.summary(np.zeros((2, 9), F32), 0.5, 2) == [0, -1, -1, 0]


def test_the_compare_is_signed_and_a_nan_is_quiet():
    x = np.zeros((2, 12), F32)
    x[0, 2] = -1.0                                              # loud, but negative: sample > level is false (:29 takes no abs)
    x[1, 4] = np.nan
    x[1, 7] = 0.6
    assert T.loud_chunks(x, 0.5, 1) == [[7, 7]]
    assert T.loud_chunks(x, -0.5, 20) == [[0, 12]]              # 0 > -0.5 in the other channel
    assert T.loud_chunks(np.array([[0.0, -0.0]], F32), 0.0, 0) == []


def test_the_end_clamp_costs_the_open_chunk_a_frame():
    # num_frames 100, the only chunk { 90, 100 } (open): cut_frames clamps the end to 99 (:219), so 9 frames, not 10
    x = _spikes(100, range(90, 100))
    assert T.loud_chunks(x, 0.5, 3) == [[90, 100]]
    cuts, fade_ins, offsets = T.fades(100, SR, [[90, 100]], 0.0)
    assert cuts == [(90, 9, 0, 0)]
    out = T.render(T.remove_silence_table(x, SR, 0.5, 3 / SR + 1e-6, 0.0), x, SR)
    assert out.shape == (1, 9)


def test_the_fades_loop_reads_what_the_iteration_before_wrote():
    # 1000 frames at 1000 Hz (a frame is a millisecond), fade 0.1 s = 100 frames, chunks { 150, 200 }, { 400, 950 }, { 960, 1000 }
    #   i = 0: 100 frames; 150 - 100 >= 0: fade_ins[0] = 0.1; 200 + 100 < 1000: fade_ins[1] = 0.1
    #   i = 1: 100 frames; fade_ins[1] = 0.1; 950 + 100 >= 1000: fade_ins[2] = ( 1000 - 950 ) / 1000 = 0.05
    #   i = 2: reads fade_ins[2] = 0.05 -> 50 frames (NOT 100); 960 - 50 >= 0: fade_ins[2] = 0.05; 1000 + 50 >= 1000: fade_ins[3] = 0
    # cuts: ( 150 - 100, 200 + 100, 100, 100 ), ( 400 - 100, 950 + 50, 100, 50 ) with the end clamped to 999, ( 960 - 50, 1000 + 0, 50, 0 ) -> 999
    cuts, fade_ins, offsets = T.fades(1000, 1000.0, [[150, 200], [400, 950], [960, 1000]], 0.1)
    assert [float(f) for f in fade_ins] == [float(F32(0.1)), float(F32(0.1)), float(F32(0.05)), 0.0]
    assert cuts == [(50, 250, 100, 100), (300, 699, 100, 50), (910, 89, 50, 0)]
    # the offsets are -2 * fade_ins[i], not -fade_ins[i]
    assert [float(o) for o in offsets] == [float(F32(-2) * F32(0.1)), float(F32(-2) * F32(0.1)), float(F32(-2) * F32(0.05)), -0.0]
    # a fade that would reach before frame 0 is the chunk's start
    cuts, fade_ins, _ = T.fades(1000, 1000.0, [[30, 200]], 0.1)
    assert float(fade_ins[0]) == float(F32(0.03)) and cuts == [(0, 300, 30, 100)]


def test_join_places_the_chunks_by_the_fp32_sum_of_lengths_and_offsets():
    # the case above joined: starts 0, 0 + 0.25 - 0.2 = 0.05 s -> frame 50 (or 49: whatever the fp32 sum truncates to), then + 0.699 - 0.1
    cuts, _, offsets = T.fades(1000, 1000.0, [[150, 200], [400, 950], [960, 1000]], 0.1)
    frames = T.join_frames([c[1] for c in cuts], offsets, 1000.0)
    t1 = F32(F32(F32(0) + F32(250) / F32(1000)) + offsets[1])
    t2 = F32(F32(t1 + F32(699) / F32(1000)) + offsets[2])
    assert frames == [0, int(F32(t1 * F32(1000))), int(F32(t2 * F32(1000)))]
    assert frames[1] in (49, 50) and frames[2] in (648, 649)


def test_edge_cut_and_splits():
    x = _spikes(100, [10, 60])
    assert T.edge_cut(x, 1000.0, 0.5, 0.0) == (10, 61, 0, 0)
    assert T.edge_cut(x, 1000.0, 0.5, 0.02) == (-10, 81, 10, 20)          # the start fade cannot reach before frame 0: it is the start frame
    assert T.edge_cut(x, 1000.0, 0.5, 0.05) == (-40, 111, 10, 39)         # the end fade: 61 + 50 >= 100: 100 - 61
    assert T.edge_cut(np.zeros((1, 100), F32), 1000.0, 0.5, 0.0) == (100, 0, 0, 0)      # nothing noisy: cut_frames( 100, 0 ): null
    assert T.split_frames(100, 1000.0, [0.05, 0.02, -1.0, 0.0, 0.2, 0.07]) == [0, 20, 50, 70, 100]        # sorted; <= 0 skipped; 0.2 s stops the list
    assert [float(t) for t in T.split_lengths_times([0.25, -1.0, 0.5])] == [0.25, 0.25, 0.75]
    assert len(T.equal_lengths(100, 1000.0, 0.03)) == 4 and T.equal_lengths(100, 1000.0, 0.0) == []


def test_boundaries_reverse_and_the_generator():
    x = np.arange(1, 11, dtype=F32).reshape(2, 5)
    assert T.reverse(x).tolist() == [[5, 4, 3, 2, 1], [10, 9, 8, 7, 6]]
    assert T.modify_boundaries(x, 1000.0, -2, 1).tolist() == [[0, 0, 1, 2, 3, 4, 5, 0], [0, 0, 6, 7, 8, 9, 10, 0]]
    assert T.modify_boundaries(x, 1000.0, 2, -1).tolist() == [[3, 4], [8, 9]]
    assert T.modify_boundaries(x, 1000.0, 3, -2) is None
    g = T.MT19937(5489)                                         # std::mt19937's default seed: its 10000th output is 4123659995 (the standard's check value)
    for _ in range(9999):
        g()
    assert g() == 4123659995
    order = T.rearrange_order(9, 1)
    assert sorted(order) == list(range(9)) and order != list(range(9)) and order == T.rearrange_order(9, 1)


def test_random_chunks_plan_counts():
    # 1024 Hz, length 0.5 s = 512 frames, chunks of 0.125 s = 128 frames (all exact in binary): the accumulator starts at 1, so a chunk starts at
    # frame 0, and it is tested BEFORE the frame's share is added, so the next start is frame 128: 0, 128, 256, 384 and the end 512
    cuts, starts, offsets, o = T.random_chunks_plan(5000, 1024.0, 0.5, 0.125, 0.0, 3)
    assert starts == [0, 128, 256, 384] and [c[1] for c in cuts] == [128] * 4 and o == [0, 128, 256, 384]
    assert all(0 <= c[0] < 5000 - 128 for c in cuts)
    # a chunk length below 32 frames is clamped to 32 frames
    _, starts, _, _ = T.random_chunks_plan(5000, 1024.0, 0.5, 0.0, 0.0, 3)
    assert starts[:3] == [0, 32, 64] and len(starts) == 16
    # a fade lengthens the cut by time_to_frame( ( fade_i + fade_i+1 ) / 2 ) and pulls the next chunk back by fade: 0.03125 s = 32 frames
    cuts, _, offsets, o = T.random_chunks_plan(5000, 1024.0, 0.5, 0.125, 0.03125, 3)
    assert [c[1:] for c in cuts] == [(160, 32, 32)] * 4 and o == [0, 128, 256, 384] and float(offsets[0]) == -0.03125
