#!/usr/bin/env python3
"""Audio::compress on the GPU: the device form (flanhip_compress_dev) timed with HIP events, median after warm-up.  8 ch x 60 s at 48 kHz:
    constant parameters        -20 dB, 3, 5 ms, 100 ms, no knee: five scalars
    per-frame parameters       five curves of n floats, already on the device
next to flanhip_copy_dev of the audio's bytes (read once, written once: what the apply pass alone has to move), flanhip_audio_gain_dev and
flanhip_audio_set_volume_dev.  Prints one JSON line per shape.

    python tools/bench_compress.py [--seconds 60] [--channels 8] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn, warmup, steps):
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(a.seconds * sr) // 4 * 4, a.channels
    amp = torch.where((torch.arange(n, device=dev) // 300) % 2 == 0, 0.5, 0.01)
    d_x = ((2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1) * amp).contiguous()
    d_out, d_gain = torch.empty_like(d_x), torch.empty(n, dtype=torch.float32, device=dev)
    d_ws = torch.empty(fa.compress_workspace_bytes(n), dtype=torch.uint8, device=dev)
    d_vol_ws = torch.empty(fa.audio_set_volume_workspace_bytes(ch, n), dtype=torch.uint8, device=dev)
    t = torch.arange(n, dtype=torch.float32, device=dev) / n
    curves = dict(threshold=(-30.0 + 20.0 * t).contiguous(), ratio=(2.0 + 4.0 * t).contiguous(), attack=(0.001 + 0.02 * t).contiguous(),
                  release=(0.05 + 0.2 * t).contiguous(), knee_width=(6.0 * t).contiguous())
    constants = dict(threshold=-20.0, ratio=3.0, attack=0.005, release=0.1, knee_width=0.0)
    moved = 8.0 * ch * n                                                # bytes: the audio read once, the result written once
    shapes = [
        ("copy (yardstick)", lambda: fa.check(fa.lib.flanhip_copy_dev(fa._dp(d_x), fa._dp(d_out), ch * n, None))),
        ("modify_volume, a curve", lambda: fa.audio_gain_dev(d_x, ch, n, d_gain, d_out)),
        ("set_volume, a scalar", lambda: fa.audio_set_volume_dev(d_x, ch, n, sr, 0.9, d_out, d_vol_ws)),
        ("compress, constant parameters", lambda: fa.compress_dev(d_x, ch, n, sr, d_x, ch, n, d_out, d_gain, d_ws, **constants)),
        ("compress, per-frame parameters", lambda: fa.compress_dev(d_x, ch, n, sr, d_x, ch, n, d_out, d_gain, d_ws, **curves)),
        ("compress, constant parameters, mono", lambda: fa.compress_dev(d_x, 1, n, sr, d_x, 1, n, d_out, d_gain, d_ws, **constants)),
    ]
    d_gain.fill_(0.5)
    for name, fn in shapes:
        med, best = timed(torch, fn, a.warmup, a.steps)
        print(json.dumps({"shape": name, "channels": ch, "frames": n, "device_ms_median": round(med, 4), "device_ms_min": round(best, 4),
                          "audio_bytes_moved": moved, "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}), flush=True)


if __name__ == "__main__":
    main()
