#!/usr/bin/env python3
"""Audio::get_local_wavelengths on the GPU: the device form (flanhip_audio_local_wavelengths_dev, one fused launch) timed with HIP events.
1 ch x 60 s at 48 kHz, resident in HBM, a 5-harmonic 220 Hz tone over a noise floor, at ( window, hop ) = ( 2048, 128 ), the API default,
and ( 1024, 128 ).  Per case: the windows, the time, windows per second, seconds of audio per second, and the launch's arithmetic by
count -- per window h^2 terms of d (h = window / 2), each an fp32 subtraction and a fused multiply-add: 3 h^2 flops -- as flops per second
and as a share of the fp32 vector peak; the split form (dprime -> pick, d' through HBM) beside it.  Every case is warmed up and then
repeated until its timed window is at least a second.  A record, not a gate.  Prints one JSON line.

    python tools/bench_pitch.py [--seconds 60] [--window 1.0] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP32_VECTOR_PEAK = 157.3e12          # flops / s, the MI355X's specification


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
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n = int(a.seconds * sr)
    t = torch.arange(n, dtype=torch.float64, device=dev) / sr
    tone = sum(torch.sin(2 * np.pi * 220.0 * k * t + k) / k for k in range(1, 6)) * (0.35 / 1.5)
    d_x = (tone + 0.02 * torch.randn(n, dtype=torch.float64, device=dev)).to(torch.float32).contiguous()
    result = {"workload": "get_local_wavelengths", "channels": 1, "frames": n, "fp32_vector_peak_flops_per_s": FP32_VECTOR_PEAK, "cases": []}
    for window, hop in ((2048, 128), (1024, 128)):
        count, h = fa.local_wavelengths_count(n, 0, -1, window, hop), window // 2
        d_out = torch.empty(count, dtype=torch.float32, device=dev)
        d_rows = torch.empty((count, h), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.local_wavelengths_workspace_bytes(n, 0, -1, window, hop), dtype=torch.uint8, device=dev)
        flops = 3.0 * h * h * count
        entry = {"window": window, "hop": hop, "windows": count, "terms_per_window": h * h, "flops_of_the_launch": flops}

        def split():
            fa.yin_dprime_dev(d_x, n, 0, -1, window, hop, d_rows)
            fa.yin_pick_dev(d_rows, count, h, 0.2, 10, d_out)
        for key, fn in (("fused", lambda: fa.local_wavelengths_dev(d_x, n, 0, -1, window, hop, 0.2, 10, d_out, d_ws)), ("split", split)):
            med, best, reps = timed(torch, fn, a.warmup, a.window)
            seconds = med * 1e-3
            entry[key] = {"device_ms_median": round(med, 4), "device_ms_min": round(best, 4), "repeats": reps,
                          "windows_per_s": round(count / seconds, 1), "audio_seconds_per_second": round(a.seconds / seconds, 1),
                          "flops_per_s": round(flops / seconds, 1), "share_of_fp32_vector_peak": round(flops / seconds / FP32_VECTOR_PEAK, 4)}
        entry["found"] = int((d_out != 0).sum().item())
        result["cases"].append(entry)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
