#!/usr/bin/env python3
"""Audio::synthesize_spectrum on the GPU: the device forms timed with HIP events, median after warm-up.
    table          flanhip_spectrum_table_dev at spectrum_size_power 16, 20 and 22 (the default Gaussian spectrum, seeded phases): the fill and
                   the two passes of the inverse transform, three launches.  Each of the three reads and writes the C = N/2 complex points once
                   (the fill reads mag and theta instead: as many bytes), so the yardstick beside it is flanhip_copy_dev of 8 C bytes -- one
                   pass's traffic -- from the same process; passes_of_copy is the table's time in units of that copy (3 if every pass ran at the
                   copy's speed)
    whole call     flanhip_audio_synthesize_spectrum_dev at the method's defaults: 2^20 table frames, fundamental 2^8, 2 channels, 10 s at 220 Hz,
                   granularity 48 frames (table, the resampler loop with its host plan, set_volume); plan_ms is one flanhip_spectrum_synth_plan
                   call timed alone, and the copy beside it moves the output's bytes
A per-kernel split comes from running this under a kernel trace (rocprofv3 --kernel-trace --stats -- python tools/bench_spectrum.py).
Prints one JSON line per shape.  No threshold.

    python tools/bench_spectrum.py [--seconds 10] [--channels 2] [--steps 20] [--warmup 3] [--powers 16 20 22]"""
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
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--powers", type=int, nargs="+", default=[16, 20, 22])
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    import spectrum_reference as R
    dev = torch.device("cuda", 0)

    def copy_ms(floats):
        src = torch.zeros(floats, dtype=torch.float32, device=dev)
        dst = torch.empty(floats, dtype=torch.float32, device=dev)
        return timed(torch, lambda: fa.check(fa.lib.flanhip_copy_dev(fa._dp(src), fa._dp(dst), floats, None)), a.warmup, a.steps)

    spectra = {}
    for p in sorted(set(a.powers + [20])):
        harmonic, _ = R.bins(p, 8)
        spectra[p] = (torch.from_numpy(R.magnitudes(p, 8)).to(dev), torch.from_numpy(R.phases(1000 + p, harmonic)).to(dev))

    for p in a.powers:
        d_mag, d_theta = spectra[p]
        N, C, _ = R.sizes(p)
        d_table = torch.empty(N, dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.spectrum_table_workspace_bytes(p), dtype=torch.uint8, device=dev)
        med, low = timed(torch, lambda: fa.spectrum_table_dev(d_mag, d_theta, p, d_table, d_ws), a.warmup, a.steps)
        cmed, clow = copy_ms(2 * C)
        print(json.dumps({"shape": "table", "spectrum_size_power": p, "complex_points": C, "launches": 3 if p > 13 else 2,
                          "device_ms_median": round(med, 4), "device_ms_min": round(low, 4), "pass_bytes_read_and_written": 8 * C,
                          "copy_of_one_pass_ms_median": round(cmed, 4), "copy_of_one_pass_ms_min": round(clow, 4),
                          "passes_of_copy": round(med / cmed, 2), "table_seconds_per_second": round(N / 48000.0 / (med * 1e-3), 1)}), flush=True)

    # the whole call at the method's defaults
    p, fp, ch, g = 20, 8, a.channels, 48
    n = int(a.seconds * 48000.0)
    freq = np.array([220.0], np.float32)
    d_mag, d_theta = spectra[p]
    t0 = time.perf_counter()
    plan = fa.spectrum_synth_plan(n, 2.0 ** fp, g, freq)
    plan_ms = (time.perf_counter() - t0) * 1e3 / 2                            # (the binding runs the plan twice: count, then fill)
    d_out = torch.empty((ch, n), dtype=torch.float32, device=dev)
    d_ws = torch.empty(fa.audio_synthesize_spectrum_workspace_bytes(p, fp, ch, n, g, freq), dtype=torch.uint8, device=dev)
    med, low = timed(torch, lambda: fa.audio_synthesize_spectrum_dev(d_mag, d_theta, p, fp, ch, n, g, freq, d_out, d_ws), a.warmup, a.steps)
    cmed, clow = copy_ms(ch * n)
    print(json.dumps({"shape": "whole call", "spectrum_size_power": p, "fundamental_power": fp, "channels": ch, "out_frames": n,
                      "blocks": int(plan["wanted"].size), "device_ms_median": round(med, 4), "device_ms_min": round(low, 4), "plan_ms": round(plan_ms, 3),
                      "copy_of_the_output_ms_median": round(cmed, 4), "audio_seconds_per_second": round(a.seconds / (med * 1e-3), 1)}), flush=True)


if __name__ == "__main__":
    main()
