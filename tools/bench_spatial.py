#!/usr/bin/env python3
"""Audio::stereo_spatialize on the GPU, stage by stage.  1 ch x 60 s at 48 kHz under three motions:
    slow orbit          radius 2 m, 0.5 Hz: ratio on both sides of 1, a table per block on the approaching half
    fly-by              30 m/s past the head at 2 m: approaching (a table per block), then receding (one table)
    constant position   the pure delay: no resampler
Per motion one JSON line: the device stages timed with HIP events, median after warm-up -- the 500 Hz low-pass
(flanhip_filter_1pole_dev), the ear kernel (flanhip_spatial_ear_dev, both ears) and the ITD launch (flanhip_spatial_itd_dev, both ears; it
runs the host plan itself before it launches, so its interval holds the plan, the upload of the records with one stream synchronisation
and the kernels) or the delay --, the host plan timed alone (flanhip_spatial_itd_plan for both ears, records kept), the bytes each stage
moves against the 8 TB/s model, and, from tests/cpp/spatial_test --bench, the whole C++ method on the wall clock with the sampling of the
position and the speed limiter timed on their own.  Both motions stay under the speed limit, so the limiter changes nothing here: its
time is the time of the pass.

    python tools/bench_spatial.py [--seconds 60] [--steps 10] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def events_ms(torch, body, warmup, steps):
    times = []
    for i in range(warmup + steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        body()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def time_plan(fa, n, sr, stretches, warmup, steps):
    """flanhip_spatial_itd_plan for every ear, records kept, into arrays allocated beforehand: median ms"""
    count = stretches.shape[1]
    kinds = (np.int64, np.float64, np.float64, np.float64, np.int32, np.int32, np.int64, np.int32, np.int32)
    arrays = [np.empty(count, k) for k in kinds]
    ptrs = [C.c_void_p(v.ctypes.data) for v in arrays]
    total = C.c_int64(0)
    times = []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        for row in stretches:
            got = fa.lib.flanhip_spatial_itd_plan(n, sr, C.c_void_p(row.ctypes.data), count, count, *ptrs, C.byref(total))
            assert got == count
        t1 = time.perf_counter()
        if i >= warmup:
            times.append((t1 - t0) * 1e3)
    return float(np.median(times))


def method_lines(seconds, steps, warmup):
    """the whole C++ method, from tests/cpp/spatial_test --bench (built as tests/test_spatial_host_cpp.py builds it)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_spatial_host_cpp as T
    T._build()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "flan_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([T.BIN, "--bench", str(seconds), str(steps), str(warmup)], capture_output=True, text=True, env=env, timeout=1200)
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 3, r.stdout + r.stderr
    return {ln["shape"]: ln for ln in lines}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    import flan_amd as fa
    import spatial_reference as S
    dev = torch.device("cuda", 0)
    sr, hw = 48000.0, 0.18
    n = int(a.seconds * sr)
    t = (np.arange(n, dtype=np.float32) * np.float32(1.0 / sr)).astype(np.float32)
    motions = [("slow orbit", np.stack([2.0 * np.cos(np.pi * t), 2.0 * np.sin(np.pi * t)], 1).astype(np.float32)),
               ("fly-by", np.stack([30.0 * (t - np.float32(a.seconds / 2)), np.full(n, 2.0, np.float32)], 1).astype(np.float32))]
    whole = method_lines(a.seconds, a.steps, a.warmup)
    d_x = (0.5 * torch.randn((1, n), dtype=torch.float32, device=dev)).contiguous()
    d_lp, d_shaped = torch.empty_like(d_x), torch.empty((2, n), dtype=torch.float32, device=dev)
    d_fws = torch.empty(fa.filter_1pole_workspace_bytes(1, n), dtype=torch.uint8, device=dev)
    lowpass_ms = events_ms(torch, lambda: fa.filter_1pole_dev(d_x, 1, n, sr, 500.0, fa.FILTER_BUTTERWORTH_LOW, 1, d_lp, d_fws), a.warmup, a.steps)
    for name, positions in motions:
        ps = positions.astype(np.float64)
        assert np.max(S.mag(np.diff(ps, axis=0))) * sr < 342.0                 # under the limit: the limiter leaves every frame as it is
        nout, stretches = zip(*(fa.spatial_itd_out_frames(n, sr, S.mag(S.relative(ps, hw, left)[::S.G])) for left in (S.LEFT, S.RIGHT)))
        stretches, stride = np.ascontiguousarray(np.stack(stretches)), max(nout)
        plan = fa.spatial_itd_plan(n, sr, stretches[0])
        plan_ms = time_plan(fa, n, sr, stretches, a.warmup, a.steps)
        d_ps = torch.from_numpy(ps).to(dev)
        d_out = torch.empty((2, stride), dtype=torch.float32, device=dev)
        d_ws = torch.empty(fa.spatial_itd_workspace_bytes(n, sr, stretches), dtype=torch.uint8, device=dev)
        ear_ms = events_ms(torch, lambda: fa.spatial_ear_dev(d_x, d_lp, n, sr, d_ps, hw, fa.SPATIAL_BOTH, d_shaped), a.warmup, a.steps)
        itd_ms = events_ms(torch, lambda: fa.spatial_itd_dev(d_shaped, 2, n, sr, stretches, list(nout), stride, d_out, d_ws), a.warmup, a.steps)
        ear_bytes, itd_bytes = 4.0 * n * 2 + 16.0 * n + 8.0 * n, 8.0 * n + 8.0 * stride
        w = whole[name]
        print(json.dumps({"shape": name, "in_frames": n, "out_frames": stride, "blocks_per_ear": int(stretches.shape[1]),
                          "tables_left_ear": int(np.unique(np.stack([plan["filtpos"], plan["oversize"].astype(np.float64)]), axis=1).shape[1]),
                          "method_ms_median": w["method_ms_median"], "sampling_ms": w["sampling_ms"], "limiter_ms": w["limiter_ms"],
                          "plan_ms_both_ears": round(plan_ms, 3), "lowpass_ms": round(lowpass_ms, 4), "ear_ms": round(ear_ms, 4),
                          "itd_launch_ms": round(itd_ms, 4), "itd_minus_plan_ms": round(itd_ms - plan_ms, 3),
                          "ear_share_of_8TBps_model": round(ear_bytes / 8e12 / (ear_ms * 1e-3), 5),
                          "itd_share_of_8TBps_model": round(itd_bytes / 8e12 / (max(itd_ms - plan_ms, 1e-6) * 1e-3), 5),
                          "audio_seconds_per_second": round(a.seconds / (w["method_ms_median"] * 1e-3), 1)}), flush=True)
    # the constant position: the ear kernel with one weight and gain per ear, then the delay
    p = np.array([2.0, 1.0])
    delays = [np.float32(np.float32(np.float32(S.mag(S.relative(p, hw, left))[0]) / S.SOUND) * np.float32(sr)) for left in (S.LEFT, S.RIGHT)]
    frames = [int(np.float32(np.float32(n) + d)) for d in delays]
    d_out = torch.empty((2, max(frames)), dtype=torch.float32, device=dev)
    ear_ms = events_ms(torch, lambda: fa.spatial_ear_dev(d_x, d_lp, n, sr, (2.0, 1.0), hw, fa.SPATIAL_BOTH, d_shaped), a.warmup, a.steps)
    delay_ms = events_ms(torch, lambda: fa.spatial_delay_dev(d_shaped, 2, n, delays, frames, max(frames), d_out), a.warmup, a.steps)
    w = whole["constant position"]
    print(json.dumps({"shape": "constant position", "in_frames": n, "out_frames": max(frames), "method_ms_median": w["method_ms_median"],
                      "lowpass_ms": round(lowpass_ms, 4), "ear_ms": round(ear_ms, 4), "delay_ms": round(delay_ms, 4),
                      "ear_share_of_8TBps_model": round(16.0 * n / 8e12 / (ear_ms * 1e-3), 5),
                      "delay_share_of_8TBps_model": round((8.0 * n + 16.0 * max(frames)) / 8e12 / (delay_ms * 1e-3), 5),
                      "audio_seconds_per_second": round(a.seconds / (w["method_ms_median"] * 1e-3), 1)}), flush=True)


if __name__ == "__main__":
    main()
