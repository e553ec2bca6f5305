#!/usr/bin/env python3
"""Audio::add_moisture, synthesize_waveform, get_total_energy and the fades on the GPU (flan_amd/csrc/volume.hip): the device forms timed with
HIP events, median after warm-up.
    add_moisture               2 ch x 10 s at 48 kHz: the x4 up-chain, k_pointwise<MoistOp> and the down-chain apart, and the three together
    synthesize_waveform        10 s at 48 kHz, oversample 16, a sine with a swept frequency curve: the scan with the phases alone, the scan with
                               the waveform fused into its replay, the 16:1 decimation, and the whole call
    get_total_energy, fade     on the 2 ch x 10 s input
For the moisture kernel and the phase replay the bytes the kernel has to move over its time are printed as a fraction of the 8 TB/s HBM
figure.  Prints one JSON line per shape.

    python tools/bench_volume.py [--seconds 10] [--channels 2] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_SECOND = 8e12


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
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sr, over = 48000.0, 4
    ch, n = a.channels, int(a.seconds * sr)
    n_over = int(fa.lib.flanhip_resample_out_frames(n, sr, sr * over))
    f32 = dict(dtype=torch.float32, device=dev)
    d_x = (2 * torch.rand((ch, n), **f32) - 1).contiguous()
    d_up, d_shaped, d_out = torch.empty((ch, n_over), **f32), torch.empty((ch, n_over), **f32), torch.empty((ch, n), **f32)
    back = int(fa.lib.flanhip_resample_out_frames(n_over, sr * over, sr))
    assert back <= n

    def up():
        fa.check(fa.lib.flanhip_resample_dev(fa._dp(d_x), ch, n, sr, sr * over, fa._dp(d_up), None))

    def shape():
        fa.audio_moisture_dev(d_up, ch, n_over, sr * over, n, sr, 0.5, 96.0, 4.0, fa.WAVEFORM_SINE, d_shaped)

    def down():
        fa.check(fa.lib.flanhip_resample_dev(fa._dp(d_shaped), ch, n_over, sr * over, sr, fa._dp(d_out), None))

    # the oscillator
    length, osc_over = float(a.seconds), 16
    frames, n_in, in_rate = fa.synthesize_waveform_frames(length, sr, osc_over)
    d_freq = (20.0 + (20000.0 - 20.0) * torch.arange(n_in, **f32) / n_in).contiguous()
    d_phases, d_wave, d_tone = torch.empty(n_in, **f32), torch.empty(n_in, **f32), torch.empty(frames, **f32)
    d_osc_ws = torch.empty(fa.osc_workspace_bytes(n_in), dtype=torch.uint8, device=dev)
    d_syn_ws = torch.empty(fa.audio_synthesize_waveform_workspace_bytes(length, sr, osc_over), dtype=torch.uint8, device=dev)

    # energy and fade
    d_energy = torch.empty(ch, **f32)
    d_e_ws = torch.empty(fa.audio_energy_workspace_bytes(ch, n), dtype=torch.uint8, device=dev)
    fade = 4800
    d_gain = torch.sqrt(torch.arange(fade, **f32) / fade).contiguous()

    pointwise_bytes = 8.0 * ch * n_over                  # the oversampled block read once, written once
    shapes = [
        ("copy of the oversampled block (yardstick)", lambda: fa.check(fa.lib.flanhip_copy_dev(fa._dp(d_up), fa._dp(d_shaped), ch * n_over // 4 * 4, None)), pointwise_bytes),
        ("add_moisture: up-chain x4", up, None),
        ("add_moisture: k_moisture", shape, pointwise_bytes),
        ("add_moisture: down-chain 4:1", down, None),
        ("add_moisture: the three stages", lambda: (up(), shape(), down()), None),
        ("synthesize_waveform: scan, phases only", lambda: fa.osc_phase_dev(d_freq, n_in, in_rate, d_phases, None, -1, d_osc_ws), 12.0 * n_in),      # the curve read twice, the phases written
        ("synthesize_waveform: scan with the sine fused", lambda: fa.osc_phase_dev(d_freq, n_in, in_rate, None, d_wave, fa.WAVEFORM_SINE, d_osc_ws), 12.0 * n_in),
        ("synthesize_waveform: waveform at given phases", lambda: fa.waveform_dev(fa.WAVEFORM_SINE, d_phases, n_in, d_wave), 8.0 * n_in),
        ("synthesize_waveform: decimation 16:1", lambda: fa.oneshot_resample_dev(d_wave, n_in, in_rate, sr, d_tone, frames), None),
        ("synthesize_waveform: the whole call", lambda: fa.audio_synthesize_waveform_dev(fa.WAVEFORM_SINE, d_freq, length, sr, osc_over, d_tone, d_syn_ws), None),
        ("get_total_energy", lambda: fa.audio_energy_dev(d_x, ch, n, d_energy, d_e_ws), 4.0 * ch * n),
        ("fade_frames, 0.1 s at either end", lambda: fa.audio_fade_dev(d_x, ch, n, d_gain, fade, d_gain, fade, d_out), 8.0 * ch * n),
        ("ring_modulate by itself", lambda: fa.audio_ring_modulate_dev(d_x, ch, n, d_up, ch, n, d_out), 12.0 * ch * n),
    ]
    up()
    for name, fn, moved in shapes:
        med, best = timed(torch, fn, a.warmup, a.steps)
        line = {"shape": name, "device_ms_median": round(med, 4), "device_ms_min": round(best, 4)}
        if moved is not None:
            line["bytes_moved"] = moved
            line["fraction_of_8TBps"] = round(moved / (med * 1e-3) / HBM_BYTES_PER_SECOND, 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
