"""Time Audio::convolve (flan_amd/csrc/conv.hip) on the MI355X: flanhip_convolve_dev with normalize on, hipEvent timing, median of the
repeats after warm-up; prints one JSON line.  Per shape: the partition P the library takes, output samples per second, the work model
(delay-line FMAs counted exactly, FFT flops as 5 C log2 C per C-point complex transform, HBM bytes of every pass) and the share of the
bound that applies (157.3 TFLOP/s fp32 vector, 8 TB/s HBM: MI355X spec).  For context, the numpy-fp32 restatement of the reference
(tests/convolve_reference.py: one D-point transform per channel) timed on the host CPU for shape C.

    python tools/bench_convolve.py [--reps 10] [--warmup 3] [--no-cpu]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SR = 48000.0
# name, channels, seconds, IR channels, IR seconds
SHAPES = [("A", 2, 60.0, 2, 3.0), ("B", 8, 60.0, 1, 0.5), ("C", 1, 10.0, 1, 10.0)]
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 8.0e12


def time_it(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def model(ch, n, irch, m, P, normalize=True):
    """work of one call with partition P (conv.hip): FMAs, flops, HBM bytes"""
    K, J = -(-m // P), -(-(n + m) // P)
    Jx = min(J, -(-n // P) + 1)
    used = min(ch, irch)
    B = P + 1
    terms = sum(min(j + 1, K) for j in range(J))                  # complex multiply-adds per (channel, bin)
    delay_fma = 4 * ch * B * terms
    transforms = used * K + ch * Jx + ch * J
    fft_flop = transforms * 5 * P * math.log2(P)
    spec = 8 * B
    hbm = (4 * ch * n + 4 * used * m                              # spectra kernels read the signals
           + spec * (used * K + ch * Jx)                          # ... and write the spectra
           + spec * (used * K + ch * Jx)                          # the delay line reads them once (re-reads: caches)
           + spec * ch * J * 2                                    # Y written, read by the inverse
           + 4 * ch * (n + m))                                    # the output
    if normalize:
        hbm += 8 * ch * (n + m)                                   # the scale pass
    return {"P": P, "K": K, "J": J, "delay_fma": delay_fma, "fft_flop": int(fft_flop),
            "flop": int(2 * delay_fma + fft_flop), "hbm_bytes": int(hbm)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    fa.check(fa.lib.flanhip_set_device(0))
    res = {"shapes": []}
    for name, ch, sec, irch, irsec in SHAPES:
        n, m = int(sec * SR), int(irsec * SR)
        x = torch.empty((ch, n), dtype=torch.float32, device=dev)
        h = torch.empty((irch, m), dtype=torch.float32, device=dev)
        fa.check(fa.lib.flanhip_noise_dev(fa._dp(x), ch, n, 7, None))
        fa.check(fa.lib.flanhip_noise_dev(fa._dp(h), irch, m, 8, None))
        out = torch.empty((ch, n + m), dtype=torch.float32, device=dev)
        ws = torch.empty((fa.convolve_workspace_bytes(ch, n, irch, m),), dtype=torch.uint8, device=dev)
        t = time_it(lambda: fa.convolve_dev(x, ch, n, h, irch, m, SR, True, out, ws), a.reps, a.warmup)
        w = model(ch, n, irch, m, fa.convolve_partition(n, m))
        t_flop, t_hbm = w["flop"] / PEAK_FLOPS, w["hbm_bytes"] / PEAK_BYTES
        bound = "fp32" if t_flop > t_hbm else "hbm"
        res["shapes"].append(dict(shape=name, channels=ch, seconds=sec, ir_channels=irch, ir_seconds=irsec, ms=round(t, 4),
                                  out_samples_per_s=round(ch * (n + m) / (t * 1e-3), 0), **w, bound=bound,
                                  bound_share=round(max(t_flop, t_hbm) / (t * 1e-3), 3)))
        del x, h, out, ws
        torch.cuda.empty_cache()
    if not a.no_cpu:
        import convolve_reference as R
        rng = np.random.default_rng(0)
        x = rng.standard_normal((1, 480000)).astype(np.float32)
        h = rng.standard_normal((1, 480000)).astype(np.float32)
        t0 = time.perf_counter()
        R.restatement(x, h, SR, normalize=True)
        res["cpu_numpy_fp32_restatement_shape_C_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
