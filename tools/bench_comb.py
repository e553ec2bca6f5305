#!/usr/bin/env python3
"""Audio::filter_comb on the GPU: the device form (flanhip_filter_comb_dev) timed with HIP events.  8 ch x 60 s at 48 kHz, resident in HBM:
    scalar      cutoff 440 Hz (d = 54.54 frames), feedback 0.7: the host knows d and launches 17 rounds, 16 work
    sweep       cutoff 200 -> 8000 Hz exponential as a curve, feedback 0.7 as a curve: 22 rounds launched
    deepest     cutoff sample_rate / 2: d = 1, one chain of n frames, every one of the 22 rounds works
    default     feedback 0 (the default), cutoff 440 Hz: the same links and rounds as `scalar`, C = 0 from the first round on
next to filter_1pole_lowpass at order 1 (one scan section: three launches) in the same process as the yardstick.  Per case: the time, the
rounds that did work (the words at the head of the workspace), the bytes the launches STREAM by the layout -- every row and plane a launch
reads or writes once, front to back -- and with them the share of the 8 TB/s HBM roofline; beside it the same with the GATHERS added, one
parent value per value streamed in, as if every frame had a live link in every working round and no parent came from a cache: the truth
lies between the two (neighbouring frames' parents are neighbours).  A round that returns at once counts no bytes.  Every case is timed twice: the
global rounds alone (the LDS level switched off by flanhip_filter_comb_debug_local) -- the bytes are counted for this form -- and the
library's choice, which runs the first rounds tile-local in LDS.  Every case is warmed up
and then repeated until its timed window is at least a second.  A record, not a gate.  Prints one JSON line.

    python tools/bench_comb.py [--seconds 60] [--channels 8] [--window 1.0] [--warmup 3]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12          # bytes / s, the MI355X's HBM3E specification


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


def layout_bytes(ch, n, rounds_done, link_curves, out_curves):
    """( streamed, streamed + gathered, streamed by one later round ) bytes of a call by the workspace layout (include/flanhip.h).
    k_comb_link reads its curves and writes a row P (4 n) and a row C (8 n).  A working round streams P, C and the planes X in (the first
    round the fp32 audio) and out, and gathers as much again as it streamed in from the parents.  k_comb_out reads its curves and u (fp64;
    with no round the audio), gathers u[p] and writes the audio's size"""
    streamed = 4 * n * link_curves + 12 * n
    gathered = 0
    for r in range(rounds_done):
        x_in = (4 if r == 0 else 8) * ch * n
        streamed += (12 * n + x_in) + (12 * n + 8 * ch * n)
        gathered += 12 * n + x_in
    streamed += 4 * n * out_curves + (8 if rounds_done else 4) * ch * n + 4 * ch * n
    gathered += 8 * ch * n if rounds_done else 0
    return streamed, streamed + gathered, 2 * (12 * n + 8 * ch * n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(a.seconds * sr) // 4 * 4, a.channels
    d_x = (2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1).contiguous()
    d_out = torch.empty_like(d_x)
    ws_bytes = fa.filter_comb_workspace_bytes(ch, n)
    d_ws = torch.empty(max(ws_bytes, fa.filter_1pole_workspace_bytes(ch, n)), dtype=torch.uint8, device=dev)
    frames = torch.arange(n, dtype=torch.float32, device=dev)
    d_sweep = (200.0 * (8000.0 / 200.0) ** (frames / n)).contiguous()
    d_k = torch.full((n,), 0.7, dtype=torch.float32, device=dev)
    yard_med, yard_min, yard_reps = timed(torch, lambda: fa.filter_1pole_dev(d_x, ch, n, sr, 1000.0, fa.FILTER_BUTTERWORTH_LOW, 1, d_out, d_ws),
                                          a.warmup, a.window)
    result = {"workload": "filter_comb", "channels": ch, "frames": n, "workspace_bytes": ws_bytes, "hbm_peak_bytes_per_s": HBM_PEAK,
              "filter_1pole_lowpass_order_1_ms_median": round(yard_med, 4), "filter_1pole_lowpass_order_1_ms_min": round(yard_min, 4),
              "filter_1pole_lowpass_order_1_repeats": yard_reps, "cases": []}

    def case(name, cutoff, feedback, link_curves, out_curves):
        fn = lambda: fa.filter_comb_dev(d_x, ch, n, sr, cutoff, feedback, 0.5, False, d_out, d_ws)      # noqa: E731
        entry = {"case": name}
        # the global rounds alone (the LDS level switched off by its hook), then the library's choice, in the same process
        for key, forced in (("global_rounds_only", -1), ("with_the_lds_level", 0)):
            with fa.filter_comb_local_forced(forced):
                med, best, reps = timed(torch, fn, a.warmup, a.window)
            head = d_ws[:256].cpu().numpy().view(np.int32)
            entry[key] = {"device_ms_median": round(med, 4), "device_ms_min": round(best, 4), "repeats": reps, "rounds": int(head[33]),
                          "a_tile_failed": bool(head[32]), "times_filter_1pole_order_1": round(med / yard_med, 2),
                          "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}
        plain = entry["global_rounds_only"]
        seconds = plain["device_ms_median"] * 1e-3
        streamed, with_gathers, per_round = layout_bytes(ch, n, plain["rounds"], link_curves, out_curves)
        plain.update({"streamed_bytes_of_a_round": per_round, "streamed_bytes_of_the_call": streamed, "streamed_bytes_per_s": round(streamed / seconds, 1),
                      "share_of_hbm_roofline": round(streamed / seconds / HBM_PEAK, 4),
                      "share_of_hbm_roofline_with_gathers": round(with_gathers / seconds / HBM_PEAK, 4),
                      "ms_per_working_round": round(plain["device_ms_median"] / max(plain["rounds"], 1), 4)})
        entry["lds_level_speedup"] = round(plain["device_ms_median"] / entry["with_the_lds_level"]["device_ms_median"], 3)
        result["cases"].append(entry)
    case("scalar: 440 Hz, feedback 0.7", 440.0, 0.7, 0, 0)
    case("sweep: 200 -> 8000 Hz curve, feedback 0.7 curve", d_sweep, d_k, 2, 1)
    case("deepest: sample_rate / 2, feedback 0.7", sr / 2, 0.7, 0, 0)
    case("default: 440 Hz, feedback 0", 440.0, 0.0, 0, 0)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
