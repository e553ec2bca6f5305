"""Time the sliding-DFT vocoder (flan_amd/csrc/spv.hip) on the MI355X: analysis and synthesis per shape, hipEvent timing after warm-up,
median of the repeats; prints one JSON line.  Algorithmic bytes: the analysis writes 8 B per MF, the synthesis reads 8 B per MF; the
fraction is of 8 TB/s.  Also a CPU figure for context: the numpy restatement's stage-3 running sum, steps per second.

    python tools/bench_spv.py [--reps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [(1, 10.0, 1024), (8, 1.0, 1024), (1, 10.0, 256)]
SR = 48000.0


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
    for ch, sec, N in SHAPES:
        n = int(sec * SR)
        x = torch.empty((ch, n), dtype=torch.float32, device=dev)
        fa.check(fa.lib.flanhip_noise_dev(fa._dp(x), ch, n, 7, None))
        spv = torch.empty((ch, n, N, 2), dtype=torch.float32, device=dev)
        out = torch.empty((ch, n), dtype=torch.float32, device=dev)
        ws = torch.empty((fa.spv_synthesize_workspace_bytes(ch, n, N, SR),), dtype=torch.uint8, device=dev)
        t_a = time_it(lambda: fa.spv_analyze_dev(x, ch, n, SR, N, spv), a.reps, a.warmup)
        t_s = time_it(lambda: fa.spv_synthesize_dev(spv, ch, n, N, SR, out, ws), a.reps, a.warmup)
        mfs = ch * n * N
        gb = 8.0 * mfs / 1e9
        res["shapes"].append({"channels": ch, "seconds": sec, "num_bins": N, "MFs": mfs,
                              "analysis_ms": round(t_a, 4), "analysis_GMF_per_s": round(mfs / t_a / 1e6, 1),
                              "analysis_frac_8TBps": round(gb / 8.0 / t_a, 3),
                              "synthesis_ms": round(t_s, 4), "synthesis_GMF_per_s": round(mfs / t_s / 1e6, 1),
                              "synthesis_frac_8TBps": round(gb / 8.0 / t_s, 3)})
        del x, spv, out, ws
        torch.cuda.empty_cache()
    if not a.no_cpu:
        import spv_reference as R
        N, n = 1024, 4800
        xx = np.random.default_rng(0).standard_normal(n).astype(np.float32)
        t0 = time.perf_counter()
        R.running_sums(xx, N)
        dt = time.perf_counter() - t0
        res["cpu_numpy_running_sum_steps_per_s"] = round(n * N / dt, 0)
        res["cpu_numpy_10s_N1024_stage3_s_est"] = round(480000 * N / (n * N / dt), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
