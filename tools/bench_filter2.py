#!/usr/bin/env python3
"""Audio::filter_2pole_lowpass and filter_2pole_highshelf on the GPU: the device form (flanhip_filter2_dev) timed with HIP events.  8 ch x
60 s at 48 kHz, resident in HBM:
    filter_2pole_lowpass, order 4      four 2-pole sections; with three scalars (no coefficient pass) and with three curves (cutoff swept
                                       200 -> 8000 Hz, damping swinging in [0.1, 0.9], a gain curve that the kind does not look at)
    filter_2pole_highshelf, order 2    two 2-pole sections with the shelf's mix; scalars and curves
next to flanhip_copy_dev of the audio's bytes (read once, written once) and to filter_1pole_lowpass at order 8 (also four 2-pole sections,
scalar R and a plain tap) in the same process as the yardsticks.  Every shape is warmed up and then repeated until its timed window is at
least a second.  Prints one JSON line.

    python tools/bench_filter2.py [--seconds 60] [--channels 8] [--window 1.0] [--warmup 5]"""
import argparse
import json
import os
import sys

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(a.seconds * sr) // 4 * 4, a.channels
    d_x = (2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1).contiguous()
    d_out = torch.empty_like(d_x)
    d_ws = torch.empty(max(fa.filter2_workspace_bytes(ch, n), fa.filter_1pole_workspace_bytes(ch, n)), dtype=torch.uint8, device=dev)
    frames = torch.arange(n, dtype=torch.float32, device=dev)
    d_sweep = (200.0 * (8000.0 / 200.0) ** (frames / n)).contiguous()
    d_damp = (0.5 + 0.4 * torch.sin(2 * np.pi * 3.0 * frames / sr)).contiguous()
    d_gain = (12.0 * torch.sin(2 * np.pi * 10.0 * frames / sr)).contiguous()
    copy_med, copy_min, copy_reps = timed(torch, lambda: fa.check(fa.lib.flanhip_copy_dev(fa._dp(d_x), fa._dp(d_out), ch * n, None)), a.warmup, a.window)
    result = {"workload": "filter_2pole", "channels": ch, "frames": n, "audio_bytes_moved_by_the_copy": 8.0 * ch * n,
              "copy_ms_median": round(copy_med, 4), "copy_ms_min": round(copy_min, 4), "copy_repeats": copy_reps, "shapes": []}

    def shape(name, sections, fn):
        med, best, reps = timed(torch, fn, a.warmup, a.window)
        result["shapes"].append({"shape": name, "sections": sections, "device_ms_median": round(med, 4), "device_ms_min": round(best, 4),
                                 "repeats": reps, "ms_per_section": round(med / sections, 4), "times_the_copy": round(med / copy_med, 2),
                                 "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)})
    shape("filter_1pole_lowpass order 8, constant", 4,
          lambda: fa.filter_1pole_dev(d_x, ch, n, sr, 1000.0, fa.FILTER_BUTTERWORTH_LOW, 8, d_out, d_ws))
    shape("filter_1pole_lowpass order 8, swept", 4,
          lambda: fa.filter_1pole_dev(d_x, ch, n, sr, d_sweep, fa.FILTER_BUTTERWORTH_LOW, 8, d_out, d_ws))
    shape("filter_2pole_lowpass order 4, scalars", 4,
          lambda: fa.filter2_dev(d_x, ch, n, sr, 1000.0, 0.5, 0.0, fa.FILTER2_LOW, 4, d_out, d_ws))
    shape("filter_2pole_lowpass order 4, three curves", 4,
          lambda: fa.filter2_dev(d_x, ch, n, sr, d_sweep, d_damp, d_gain, fa.FILTER2_LOW, 4, d_out, d_ws))
    shape("filter_2pole_highshelf order 2, scalars", 2,
          lambda: fa.filter2_dev(d_x, ch, n, sr, 1000.0, 0.5, 6.0, fa.FILTER2_HIGHSHELF, 2, d_out, d_ws))
    shape("filter_2pole_highshelf order 2, three curves", 2,
          lambda: fa.filter2_dev(d_x, ch, n, sr, d_sweep, d_damp, d_gain, fa.FILTER2_HIGHSHELF, 2, d_out, d_ws))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
