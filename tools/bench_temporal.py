#!/usr/bin/env python3
"""Audio silence removal and reverse on the GPU (flan_amd/csrc/temporal.hip) timed with HIP events, the audio resident in HBM.  Cases: 8 ch x
60 s and 2 ch x 600 s at 48 kHz of gated noise, bursts of 50 ... 500 ms separated by silences of 20 ... 800 ms.  Columns:

  detect           flanhip_loud_summary_dev, the 32-byte read-back of the summary, flanhip_loud_chunks_dev into a table of that size, and the
                   table's read-back: what get_loud_chunks does before it cuts
  remove_silence   the whole method as Audio::remove_silence makes it: detect, the fades plan and the mix's plan on the host, one
                   flanhip_grains_mix_dev over the source; no chunk is written
  reverse          flanhip_audio_reverse_dev

Per column: the median and the minimum of repeats that fill a timed window of at least a second after warm-ups, beside its traffic floor --
bytes read plus written over the box's copy rate: --copy-gbs, the "copy_peak_measured" of `bench.py --full` (flanhip_copy_dev, bytes read +
written), or without it the same measurement taken here on two 512 MiB buffers.  detect reads the audio once and writes and reads one 8-byte
mask per lane; remove_silence adds the source bytes under the events and the output.  A record, not a gate.  Prints one JSON line.

    python tools/bench_temporal.py [--window 1.0] [--warmup 3] [--copy-gbs GB/s]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_grains import copy_rate, timed      # noqa: E402


def gate(n, sr, seed):
    """1 inside a burst, 0 in a silence: bursts of 50 ... 500 ms, silences of 20 ... 800 ms"""
    rng = np.random.default_rng(seed)
    g = np.zeros(n, np.float32)
    at = int(rng.uniform(0.02, 0.8) * sr)
    while at < n:
        burst = int(rng.uniform(0.05, 0.5) * sr)
        g[at:at + burst] = 1.0
        at += burst + int(rng.uniform(0.02, 0.8) * sr)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-gbs", type=float, default=0.0, help="the copy rate the traffic floors are taken over (bench.py --full's copy_peak_measured); 0: measured here")
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr, level, gap_time, fade = 48000.0, 0.01, 0.01, 0.002
    gap = int(np.float32(gap_time) * np.float32(sr))
    measured = copy_rate(torch, fa, dev)
    copy_gbs = a.copy_gbs or measured
    result = {"workload": "temporal", "sample_rate": sr, "level": level, "minimum_gap_s": gap_time, "fade_s": fade, "copy_rate_gb_per_s": round(copy_gbs, 1),
              "copy_rate_measured_here_gb_per_s": round(measured, 1), "run_frames": fa.loud_run_frames(), "block_frames": fa.loud_block_frames(), "cases": {}}

    for ch, seconds in ((8, 60.0), (2, 600.0)):
        n = int(seconds * sr)
        g = torch.from_numpy(gate(n, sr, ch)).to(dev)
        d_x = (0.1 * torch.randn((ch, n), dtype=torch.float32, device=dev) * g).contiguous()
        del g
        d_ws = torch.empty(fa.loud_workspace_bytes(ch, n), dtype=torch.uint8, device=dev)
        d_summary = torch.empty(4, dtype=torch.int64, device=dev)
        state = {}

        def detect():
            fa.loud_summary_dev(d_x, ch, n, level, gap, d_summary, d_ws)
            summary = d_summary.cpu().numpy()                   # the read-back that sizes the table
            count = int(summary[0])
            d_chunks = torch.empty((max(count, 1), 2), dtype=torch.int32, device=dev)
            fa.loud_chunks_dev(ch, n, gap, count, d_chunks, count, d_ws)
            state["chunks"], state["summary"] = d_chunks.cpu().numpy()[:count], summary
            return state["chunks"]

        def remove_silence():
            chunks = detect()
            events, _ = fa.loud_chunks_fades(n, sr, chunks, fade, join=True)
            events["src"], events["ch_stride"], events["src_frames"], events["channels"] = d_x.data_ptr(), n, n, ch
            frames, first, last = fa.grains_plan(events)
            d_out = torch.empty((ch, frames), dtype=torch.float32, device=dev)
            d_mix_ws = torch.empty(fa.grains_workspace_bytes(len(events), frames), dtype=torch.uint8, device=dev)
            fa.grains_mix_dev(events, first, last, None, 0, None, 0, ch, frames, sr, d_out, d_mix_ws)
            state["events"], state["frames"] = events, frames
            return d_out

        d_rev = torch.empty_like(d_x)

        def reverse():
            fa.audio_reverse_dev(d_x, ch, n, d_rev)

        remove_silence()
        torch.cuda.synchronize()
        events, frames, count = state["events"], state["frames"], len(state["chunks"])
        audio_bytes = ch * n * 4
        mask_bytes = -(-n // fa.loud_run_frames()) * 8
        floors = {"detect": audio_bytes + 2 * mask_bytes + count * 8}
        floors["remove_silence"] = floors["detect"] + int(events["n"].astype(np.int64).sum()) * ch * 4 + ch * frames * 4
        floors["reverse"] = 2 * audio_bytes
        entry = {"channels": ch, "frames": n, "chunks": count, "out_frames": int(frames)}
        for name, fn in (("detect", detect), ("remove_silence", remove_silence), ("reverse", reverse)):
            med, best, reps = timed(torch, fn, a.warmup, a.window)
            floor_ms = floors[name] / (copy_gbs * 1e9) * 1e3
            entry[name] = {"device_ms_median": round(med, 4), "device_ms_min": round(best, 4), "repeats": reps, "traffic_bytes": int(floors[name]),
                           "traffic_floor_ms": round(floor_ms, 4), "times_the_traffic_floor": round(med / floor_ms, 2),
                           "audio_seconds_per_second": round(seconds / (med * 1e-3), 1)}
        result["cases"]["%dch_%ds" % (ch, int(seconds))] = entry
        del d_x, d_rev, d_ws
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
