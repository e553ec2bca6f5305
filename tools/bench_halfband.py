#!/usr/bin/env python3
"""Audio::halfband_modulate, the modulation of shift_frequency and halfband_multiply on the GPU: the device forms (flanhip_halfband_*_dev,
flanhip_hilbert_dev) timed with HIP events.  8 ch x 60 s at 48 kHz, resident in HBM:
    halfband_modulate, rows            both cascades of the network and out = first re - second im in four launches; re and im curves
    halfband_modulate, scalars         the same with a constant modulator
    halfband_modulate, phase           the modulator exp( i phase ) of shift_frequency: cos and sin in fp64 per sample
    hilbert                            both outputs written
    halfband_multiply                  two operands, four cascades and the product
next to the yardsticks in the same process: flanhip_filter_1pole_dev REPEAT_LOW with 20 repeats on the same buffer (20 one-pole sections
through the per-section machinery: the launches and the traffic of the network unfused) and flanhip_copy_dev of the audio's bytes (read
once, written once).  Every shape is warmed up and then repeated until its timed window is at least a second.  Prints one JSON line.

    python tools/bench_halfband.py [--seconds 60] [--channels 8] [--window 1.0] [--warmup 5]

The kernels' own times (k_hb_table, k_hb_sum, k_hb_carry, k_hb_replay) come from a kernel trace of --profile, which makes 20 calls of
halfband_modulate with rows and nothing else, and --stats, which reads the trace's summary:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_halfband.py --profile
    python tools/bench_halfband.py --stats DIR"""
import argparse
import csv
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


def kernel_stats(directory):
    """the k_hb_* rows of a rocprofv3 --stats summary under `directory`: { kernel: { calls, average_us, percent } }"""
    out = {}
    for base, _, files in os.walk(directory):
        for name in files:
            if not name.endswith("kernel_stats.csv"):
                continue
            with open(os.path.join(base, name), newline="") as fh:
                for row in csv.DictReader(fh):
                    kernel = row.get("Name", "")
                    if "k_hb_" not in kernel:
                        continue
                    short = kernel[kernel.index("k_hb_"):].split("<")[0].split("(")[0]
                    e = out.setdefault(short, {"calls": 0, "total_us": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_us"] += float(row["TotalDurationNs"]) * 1e-3
    total = sum(e["total_us"] for e in out.values())
    for e in out.values():
        e["average_us"] = round(e["total_us"] / max(e["calls"], 1), 2)
        e["percent_of_the_call"] = round(100.0 * e["total_us"] / total, 2) if total else 0.0
        e["total_us"] = round(e["total_us"], 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="20 calls of halfband_modulate with rows, for a kernel trace")
    ap.add_argument("--stats", metavar="DIR", help="summarise the k_hb_* kernels of a rocprofv3 --stats run")
    a = ap.parse_args()
    if a.stats:
        print(json.dumps({"workload": "halfband_kernels", "kernels": kernel_stats(a.stats)}), flush=True)
        return
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(a.seconds * sr) // 4 * 4, a.channels
    d_x = (2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1).contiguous()
    d_b = (2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1).contiguous()
    d_out, d_out2 = torch.empty_like(d_x), torch.empty_like(d_x)
    d_ws = torch.empty(max(fa.halfband_workspace_bytes(ch, n), fa.filter_1pole_workspace_bytes(ch, n)), dtype=torch.uint8, device=dev)
    frames = torch.arange(n, dtype=torch.float32, device=dev)
    d_re = torch.cos(2 * np.pi * 250.0 * frames / sr).contiguous()
    d_im = torch.sin(2 * np.pi * 250.0 * frames / sr).contiguous()
    d_phase = torch.remainder(2 * np.pi * 250.0 * frames / sr, 2 * np.pi).contiguous()
    if a.profile:
        for _ in range(20):
            fa.halfband_modulate_dev(d_x, ch, n, sr, d_re, d_im, None, d_out, d_ws)
        torch.cuda.synchronize()
        return
    copy_med, copy_min, copy_reps = timed(torch, lambda: fa.check(fa.lib.flanhip_copy_dev(fa._dp(d_x), fa._dp(d_out), ch * n, None)), a.warmup, a.window)
    chain_med, chain_min, chain_reps = timed(torch, lambda: fa.filter_1pole_dev(d_x, ch, n, sr, 1000.0, fa.FILTER_REPEAT_LOW, 20, d_out, d_ws), a.warmup, a.window)
    result = {"workload": "halfband", "channels": ch, "frames": n, "audio_bytes_moved_by_the_copy": 8.0 * ch * n,
              "copy_ms_median": round(copy_med, 4), "copy_ms_min": round(copy_min, 4), "copy_repeats": copy_reps,
              "chain_of_20_sections_ms_median": round(chain_med, 4), "chain_of_20_sections_ms_min": round(chain_min, 4), "chain_repeats": chain_reps,
              "shapes": []}

    def shape(name, fn):
        med, best, reps = timed(torch, fn, a.warmup, a.window)
        result["shapes"].append({"shape": name, "device_ms_median": round(med, 4), "device_ms_min": round(best, 4), "repeats": reps,
                                 "times_the_copy": round(med / copy_med, 2), "chain_over_this": round(chain_med / med, 2),
                                 "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)})
    shape("halfband_modulate, rows", lambda: fa.halfband_modulate_dev(d_x, ch, n, sr, d_re, d_im, None, d_out, d_ws))
    shape("halfband_modulate, scalars", lambda: fa.halfband_modulate_dev(d_x, ch, n, sr, 0.6, -0.8, None, d_out, d_ws))
    shape("halfband_modulate, phase", lambda: fa.halfband_modulate_dev(d_x, ch, n, sr, 0.0, 0.0, d_phase, d_out, d_ws))
    shape("hilbert", lambda: fa.hilbert_dev(d_x, ch, n, sr, d_out, d_out2, d_ws))
    shape("halfband_multiply", lambda: fa.halfband_multiply_dev(d_x, ch, n, sr, d_b, ch, n, 44100.0, d_out, d_ws))
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
