#!/usr/bin/env python3
"""Audio::filter_1pole_multinotch / filter_2pole_multinotch on the GPU: the device form (flanhip_multinotch_dev) timed with HIP events.
8 ch x 60 s at 48 kHz, resident in HBM; 1-pole orders 4, 8, 16 and 2-pole orders 2, 4, 8 (4, 8 and 16 states), each with
    sweep       a cutoff curve 200 -> 8000 Hz, scalar damping 0.7, feedback 0.7 and wet_dry 0.5
    curves      every parameter a curve
Two yardsticks run INTERLEAVED with every case in the same process, one call of each per repeat: flanhip_copy_dev of the same bytes, and
flanhip_filter_1pole_dev REPEAT_LOW with as many sections as the multinotch has (the same kind of cascade without the coupling: `order`
separate scans, three launches each).  Every shape is warmed up, then the triple is repeated until the multinotch's times add up to the window
(at least 5 repeats).  Medians and the ratios to both yardsticks per case.  A record, not a gate.  Prints one JSON line.

    python tools/bench_multinotch.py [--seconds 60] [--channels 8] [--window 1.0] [--warmup 2] [--only 1pole:16]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def interleaved(torch, fns, warmup, window_s):
    """per-call device times of every fn, one call of each per repeat, until the LAST fn's times add up to the window: ( medians, repeats )"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    while (sum(times[-1]) < window_s * 1e3 or len(times[-1]) < 5) and len(times[-1]) < 200:
        for t, fn in zip(times, fns):
            t.append(once(torch, fn))
    return [float(np.median(t)) for t in times], len(times[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="kind:order, e.g. 1pole:16")
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(a.seconds * sr) // 4 * 4, a.channels
    d_x = (0.6 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 0.3).contiguous()
    d_out, d_yard = torch.empty_like(d_x), torch.empty_like(d_x)
    t = torch.arange(n, dtype=torch.float32, device=dev) / n
    d_sweep = (200.0 * (8000.0 / 200.0) ** t).contiguous()
    d_damp, d_k, d_mix = (0.2 + 1.3 * t).contiguous(), (0.9 - 1.8 * t).contiguous(), t.contiguous()
    shapes = [("1pole", fa.MULTINOTCH_1POLE, o) for o in (4, 8, 16)] + [("2pole", fa.MULTINOTCH_2POLE, o) for o in (2, 4, 8)]
    if a.only:
        shapes = [s for s in shapes if "%s:%d" % (s[0], s[2]) == a.only]
    ws_bytes = max([fa.multinotch_workspace_bytes(ch, n, kind, order) for _, kind, order in shapes] + [fa.filter_1pole_workspace_bytes(ch, n)])
    d_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    result = {"workload": "multinotch", "channels": ch, "frames": n, "audio_bytes": 4 * ch * n, "cases": []}
    copy = lambda: fa.check(fa.lib.flanhip_copy_dev(d_x.data_ptr(), d_out.data_ptr(), ch * n, None))      # noqa: E731
    for label, kind, order in shapes:
        for inputs, par in (("sweep", (d_sweep, 0.7, 0.7, 0.5)), ("curves", (d_sweep, d_damp, d_k, d_mix))):
            yard = lambda: fa.filter_1pole_dev(d_x, ch, n, sr, par[0], fa.FILTER_REPEAT_LOW, order, d_yard, d_ws)      # noqa: E731
            mn = lambda: fa.multinotch_dev(d_x, ch, n, sr, *par, kind, order, False, d_out, d_ws)      # noqa: E731
            (copy_ms, yard_ms, mn_ms), reps = interleaved(torch, (copy, yard, mn), a.warmup, a.window)
            result["cases"].append({"kind": label, "order": order, "states": order * (kind + 1), "inputs": inputs, "repeats": reps,
                                    "multinotch_ms_median": round(mn_ms, 4), "copy_ms_median": round(copy_ms, 4),
                                    "filter_1pole_repeat_low_ms_median": round(yard_ms, 4), "times_copy": round(mn_ms / copy_ms, 1),
                                    "times_filter_1pole_repeat_low": round(mn_ms / yard_ms, 2),
                                    "audio_seconds_per_second": round(ch * a.seconds / (mn_ms * 1e-3), 1),
                                    "workspace_bytes": fa.multinotch_workspace_bytes(ch, n, kind, order)})
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
