#!/usr/bin/env python3
"""Audio::mix with grains cut in flight on the GPU (flanhip_grains_mix_dev) timed with HIP events.  2 ch x 60 s at 48 kHz resident in HBM:

  fused      granulate: 2000 grains / s of 50 ms with 5 ms fades, read from a time selection that runs through the source: ~100 grains deep
             on every output sample, one launch over the source
  general    the same table with the grains materialised first: one launch cuts and fades every grain into a buffer of its own (all of them
             in one long block, back to back: the cheapest way to materialise them; the C++ general path pays a launch per grain on top), a
             second launch mixes the buffers
  mix        plain mix of 16 one-minute stereo sources a tenth of a second apart, constant gains

A call is timed whole: the table's and the plan's copies into the workspace ride on the same stream.  Per case: the median and the minimum of
repeats that fill a timed window of at least a second after warm-ups, the host time of the plan, the traffic floor -- the source bytes under
all events plus the output written, over the box's copy rate: --copy-gbs, the "copy_peak_measured" of `bench.py --full` (flanhip_copy_dev,
bytes read + written), or without it the same measurement taken here on two 512 MiB buffers -- and the ratio of fused to general.  A record,
not a gate.  Prints one JSON line.

    python tools/bench_grains.py [--seconds 60] [--window 1.0] [--warmup 3] [--copy-gbs GB/s]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, warmup, window_s):
    """( median ms, min ms, repeats ): per-call device times, repeated until they add up to the window"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    while sum(times) < window_s * 1e3 or len(times) < 5:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), len(times)


def copy_rate(torch, fa, dev, floats=1 << 27):
    """GB/s of flanhip_copy_dev, bytes read + written, best of three runs of ten (bench.py's measurement)"""
    src = torch.zeros(floats, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    args = (ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), floats, ctypes.c_void_p(0))
    fa.check(fa.lib.flanhip_copy_dev(*args))
    best = None
    for _ in range(3):
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        for _ in range(10):
            fa.check(fa.lib.flanhip_copy_dev(*args))
        c1.record()
        torch.cuda.synchronize()
        t = c0.elapsed_time(c1) / 10
        best = t if best is None else min(best, t)
    return 2 * floats * 4 / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-gbs", type=float, default=0.0, help="the copy rate the traffic floors are taken over (bench.py --full's copy_peak_measured); 0: measured here")
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr, ch = 48000.0, 2
    n = int(a.seconds * sr)
    d_src = (0.1 * torch.randn((ch, n), dtype=torch.float32, device=dev)).contiguous()
    measured = copy_rate(torch, fa, dev)
    copy_gbs = a.copy_gbs or measured
    result = {"workload": "grains_mix", "channels": ch, "frames": n, "copy_rate_gb_per_s": round(copy_gbs, 1), "copy_rate_measured_here_gb_per_s": round(measured, 1), "tile_frames": fa.grains_tile_frames(),
              "batch_events": fa.grains_batch_events(), "cases": {}}

    def case(events, d_sources, sources_floats, frames=0):
        """the plan and a closure that runs one call; ( run, frames, entry )"""
        t0 = time.perf_counter()
        frames, first, last = fa.grains_plan(events, frames)
        plan_ms = (time.perf_counter() - t0) * 1e3
        d_out = torch.empty((ch, frames), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.grains_workspace_bytes(len(events), frames), dtype=torch.uint8, device=dev)
        live = events[events["n"] > 0]
        source_bytes = int((live["n"].astype(np.int64) * live["channels"]).sum()) * 4
        out_bytes = ch * frames * 4
        entry = {"events": int(len(events)), "out_frames": int(frames), "depth": round(float(live["n"].sum()) / frames, 1), "host_plan_ms": round(plan_ms, 3),
                 "table_bytes": int(events.nbytes + first.nbytes + last.nbytes), "source_bytes_under_events": source_bytes, "output_bytes": out_bytes,
                 "traffic_floor_ms": round((source_bytes + out_bytes) / (copy_gbs * 1e9) * 1e3, 4)}
        return (lambda: fa.grains_mix_dev(events, first, last, None, 0, d_sources, sources_floats, ch, frames, sr, d_out, d_ws)), d_out, entry

    def finish(entry, run):
        med, best, reps = timed(torch, run, a.warmup, a.window)
        entry.update({"device_ms_median": round(med, 4), "device_ms_min": round(best, 4), "repeats": reps,
                      "times_the_traffic_floor": round(med / entry["traffic_floor_ms"], 2), "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)})
        return med

    # granulate: 2000 grains / s of 50 ms
    frames = fa.grains_events(n, sr, 2000.0)
    t = frames.astype(np.float32) / np.float32(sr)
    start = (t * np.float32(0.9)).astype(np.float32)
    events = fa.grains_cut(n, sr, start, (start + np.float32(0.05)).astype(np.float32), np.full(t.size, 0.005, np.float32), np.full(t.size, 0.005, np.float32))
    events["o"], events["ch_stride"], events["src_frames"], events["channels"], events["gain_offset"], events["gain"] = frames, n, n, ch, -1, 0.1
    run, d_fused, entry = case(events, d_src, ch * n)
    fused = finish(entry, run)
    result["cases"]["fused_granulate"] = entry

    # the same table through materialised grains: grain k whole at frame k * longest of one long block, then a mix of plain events over it
    longest = int(events["n"].max())
    cutting = events.copy()
    cutting["o"], cutting["gain"] = np.arange(len(events), dtype=np.int64) * longest, 1.0
    run_cut, d_grains, entry_cut = case(cutting, d_src, ch * n, frames=len(events) * longest)
    block = len(events) * longest
    mixing = events.copy()
    mixing["src"], mixing["ch_stride"], mixing["src_frames"] = np.arange(len(events), dtype=np.uint64) * np.uint64(longest), block, longest
    mixing["s"], mixing["sf"], mixing["ef"] = 0, 0, 0
    run_mix, d_general, entry_mix = case(mixing, d_grains, ch * block)
    cut_ms, mix_ms = finish(entry_cut, run_cut), finish(entry_mix, run_mix)
    torch.cuda.synchronize()
    result["cases"]["general_granulate"] = {"materialise": entry_cut, "mix": entry_mix, "device_ms_median": round(cut_ms + mix_ms, 4),
                                            "bit_identical_to_fused": bool(torch.equal(d_fused, d_general))}
    result["fused_over_general"] = round(fused / (cut_ms + mix_ms), 4)
    del d_grains, d_general

    # plain mix of 16 one-minute sources
    d_many = (0.1 * torch.randn((16, ch, n), dtype=torch.float32, device=dev)).contiguous()
    plain = np.zeros(16, fa.GRAIN_EVENT)
    plain["src"], plain["ch_stride"], plain["src_frames"], plain["n"], plain["channels"] = np.arange(16, dtype=np.uint64) * np.uint64(ch * n), n, n, n, ch
    plain["o"], plain["gain_offset"], plain["gain"] = np.arange(16) * 4800, -1, 0.25
    run, _, entry = case(plain, d_many, 16 * ch * n)
    finish(entry, run)
    result["cases"]["mix_16_sources"] = entry
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
