#!/usr/bin/env python3
"""flan::Wavetable on the GPU: the device forms timed with HIP events, median after warm-up.
    construction   a mono minute of a 220 Hz tone at 48 kHz cut every 218 frames (about 13 000 waveforms), W = 2048:
                   flanhip_wavetable_resample_dev (host record building, one upload with a stream synchronisation, k_wt_resample)
    synthesis      8 ch x 60 s at g = 48 from a 64-slot table of W = 2048, flanhip_wavetable_synth_dev (the host plan, the upload of its
                   records, k_wt_synth): once with a constant frequency (one coefficient table shared by every run) and once with a
                   sweep (a table per block); plan_ms is one flanhip_wavetable_synth_plan call timed alone
    yardstick      k_repitch_sinc (flanhip_audio_repitch_dev) at the same output count and channels, from the same process
Prints one JSON line per shape.

    python tools/bench_wavetable.py [--seconds 60] [--channels 8] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(torch, call, warmup, steps):
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    import repitch_reference as RP
    dev = torch.device("cuda", 0)
    sr, g, W = 48000.0, 48, 2048
    n, ch = int(a.seconds * sr), a.channels

    # construction
    t = np.arange(n) / sr
    x = (0.5 * np.sin(2 * np.pi * 220.0 * t) + 0.25 * np.sin(2 * np.pi * 440.0 * t + 1.1)).astype(np.float32)[None, :]
    starts = [np.arange(0, n - 218, 218, dtype=np.int32)]
    slots = fa.wavetable_slots(starts)
    d_x = torch.from_numpy(x).to(dev)
    d_table = torch.empty((1, slots * W), dtype=torch.float32, device=dev)
    d_ws = torch.empty(max(fa.wavetable_resample_workspace_bytes(1, n, starts, W), 16), dtype=torch.uint8, device=dev)
    med, low = timed(torch, lambda: fa.wavetable_resample_dev(d_x, 1, n, starts, W, d_table, None, d_ws), a.warmup, a.steps)
    print(json.dumps({"shape": "construction", "waveforms": int(slots - 1), "source_frames": n, "wavelength": W, "device_ms_median": round(med, 4),
                      "device_ms_min": round(low, 4), "waveforms_per_ms": round((slots - 1) / med, 1),
                      "table_bytes": 4 * slots * W, "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}), flush=True)

    # synthesis
    table_slots = 64
    table = (0.5 * torch.randn((ch, table_slots * W), dtype=torch.float32, device=dev)).contiguous()
    d_out = torch.empty((ch, n), dtype=torch.float32, device=dev)
    for name, freq in (("synthesis, constant 220 Hz", np.array([220.0], np.float32)),
                       ("synthesis, sweep 110 -> 440 Hz", (110.0 + 330.0 * np.arange(n) / max(n - 1, 1)).astype(np.float32))):
        t0 = time.perf_counter()
        plan = fa.wavetable_synth_plan(n, sr, W, g, freq)
        plan_ms = (time.perf_counter() - t0) * 1e3 / 2                        # (the binding runs the plan twice: count, then fill)
        blocks = plan["wanted"].size
        index = np.ascontiguousarray(np.tile(((table_slots - 1) * plan["first_out"] / n).astype(np.float32), (ch, 1)))
        d_ws = torch.empty(fa.wavetable_synth_workspace_bytes(ch, n, sr, W, g, freq), dtype=torch.uint8, device=dev)
        med, low = timed(torch, lambda: fa.wavetable_synth_dev(table, ch, table_slots, W, sr, n, g, freq, index, True, d_out, d_ws), a.warmup, a.steps)
        print(json.dumps({"shape": name, "channels": ch, "out_frames": n, "blocks": int(blocks),
                          "tables": int(np.unique(np.stack([plan["filtpos"], plan["oversize"].astype(np.float64)]), axis=1).shape[1]),
                          "device_ms_median": round(med, 4), "device_ms_min": round(low, 4), "plan_ms": round(plan_ms, 3),
                          "device_minus_plan_ms": round(med - plan_ms, 3), "ms_per_million_output_frames": round(med / (ch * n / 1e6), 4),
                          "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}), flush=True)

    # the yardstick: Audio::repitch's kernel at the same output count (a constant factor of 1: as many frames out as in)
    count = RP.factor_count(n, g)
    for name, factors in (("k_repitch_sinc, constant 1.5", np.full(count, 1.5, np.float32)),
                          ("k_repitch_sinc, sweep 0.5 -> 2", (0.5 + 1.5 * np.arange(count) / max(count - 1, 1)).astype(np.float32))):
        inv = np.ascontiguousarray(RP.invert(factors), np.float32)
        nout = fa.audio_repitch_out_frames(inv, g)
        d_in = (0.5 * torch.randn((ch, n), dtype=torch.float32, device=dev)).contiguous()
        d_y = torch.empty((ch, nout), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.audio_repitch_workspace_bytes(n, sr, inv, g), dtype=torch.uint8, device=dev)
        med, low = timed(torch, lambda: fa.audio_repitch_dev(d_in, ch, n, sr, inv, g, fa.REPITCH_SINC, d_y, d_ws), a.warmup, a.steps)
        print(json.dumps({"shape": name, "channels": ch, "out_frames": int(nout), "device_ms_median": round(med, 4), "device_ms_min": round(low, 4),
                          "ms_per_million_output_frames": round(med / (ch * nout / 1e6), 4)}), flush=True)


if __name__ == "__main__":
    main()
