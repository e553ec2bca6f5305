#!/usr/bin/env python3
"""Audio::repitch on the GPU: the device form (flanhip_audio_repitch_dev) timed with HIP events, median after warm-up, and the host
plan timed on its own.  8 ch x 60 s at 48 kHz at the default granularity (1 ms = 48 frames):
    factor 1.5 constant   one table shared by every run
    sweep 0.5 -> 2        a table per block while the pitch goes up
    factor 0.5            "ideal": one 64-tap sum per sample
Prints one JSON line per shape.  flanhip_audio_repitch_dev runs the host plan itself before it launches, so the event interval holds the
plan (the device waits for it), the upload of its records (56 bytes per block) with one stream synchronisation, and the kernels; plan_ms is
one flanhip_audio_repitch_plan call timed alone (records kept, output arrays allocated beforehand, median after warm-up), and
device_minus_plan_ms what is left for run building, upload and kernels.

    python tools/bench_repitch.py [--seconds 60] [--channels 8] [--steps 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def time_plan(fa, n, sr, inv, g, plan, warmup, steps):
    """One flanhip_audio_repitch_plan call that keeps its records, as the device form runs it, into arrays allocated beforehand: median ms."""
    import ctypes as C
    arrays = [np.empty_like(plan[k]) for k in ("offset", "fracpos", "ratio", "filtpos", "oversize", "ideal", "first_out", "wanted")]
    ptrs = [C.c_void_p(v.ctypes.data) for v in arrays]
    inv_p, nout, blocks = C.c_void_p(inv.ctypes.data), C.c_int64(0), arrays[0].size
    times = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        got = fa.lib.flanhip_audio_repitch_plan(n, sr, inv_p, inv.size, g, fa.REPITCH_SINC, blocks, *ptrs, C.byref(nout))
        t1 = time.perf_counter()
        assert got == blocks
        if i >= warmup:
            times.append((t1 - t0) * 1e3)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    import repitch_reference as R
    dev = torch.device("cuda", 0)
    sr, g = 48000.0, 48
    n, ch = int(a.seconds * sr), a.channels
    count = R.factor_count(n, g)
    shapes = [("constant 1.5", np.full(count, 1.5, np.float32)),
              ("sweep 0.5 -> 2", (0.5 + 1.5 * np.arange(count) / max(count - 1, 1)).astype(np.float32)),
              ("constant 0.5 (ideal)", np.full(count, 0.5, np.float32))]
    d_x = (0.5 * torch.randn((ch, n), dtype=torch.float32, device=dev)).contiguous()
    for name, factors in shapes:
        inv = np.ascontiguousarray(R.invert(factors), np.float32)
        plan = fa.audio_repitch_plan(n, sr, inv, g)
        nout = plan["out_frames"]
        plan_ms = time_plan(fa, n, sr, inv, g, plan, a.warmup, a.steps)
        d_out = torch.empty((ch, nout), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.audio_repitch_workspace_bytes(n, sr, inv, g), dtype=torch.uint8, device=dev)
        times = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fa.audio_repitch_dev(d_x, ch, n, sr, inv, g, fa.REPITCH_SINC, d_out, d_ws)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        med = float(np.median(times))
        moved = 4.0 * ch * (n + nout)                                      # bytes: the input read once, the output written once
        print(json.dumps({"shape": name, "channels": ch, "in_frames": n, "out_frames": nout, "blocks": int(plan["wanted"].size),
                          "tables": int(np.unique(np.stack([plan["filtpos"], plan["oversize"].astype(np.float64)]), axis=1).shape[1]),
                          "device_ms_median": round(med, 4), "device_ms_min": round(float(min(times)), 4), "plan_ms": round(plan_ms, 3), "device_minus_plan_ms": round(med - plan_ms, 3),
                          "bytes_moved": moved, "share_of_8TBps_model": round(moved / 8e12 / (med * 1e-3), 5),
                          "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}), flush=True)


if __name__ == "__main__":
    main()
