#!/usr/bin/env python3
"""A/B of TWO BUILDS of libflanhip.so on the scans over frames (compress.hip, filter.hip; run_scan.h), in one process.

    python tools/ab_scans.py [--a flan_amd/libflanhip_base.so] [--b flan_amd/libflanhip.so] [--rounds 9] [--window 1.0] [--out FILE]

Bits: compress and filter_1pole on every case of tests/compress_reference.py and tests/filter_reference.py, the host form and the _dev form
(workspace filled with 0xFF, outputs with NaN) at the default run and at forced runs 1, 7 and 64: B's output -- and the compressor's gain
curve -- against A's as 32-bit words.  A tool, not a test: it judges one build against another, the tests judge the device against the
restatements.
Times: the _dev forms on the shapes of tools/bench_compress.py and tools/bench_filter.py (8 ch x 60 s at 48 kHz; the compressor with
constant and per-frame parameters, the Butterworth low-pass at orders 1, 2 and 8 with a constant and a swept cutoff), HIP events per call,
warmed up, in rounds that alternate A, B, B, A; a round times a shape until the calls' device times (the events', not the wall clock: the
host's synchronize and the events themselves come on top) have added up to a second and keeps their median.  Per
shape: each build's median of round medians, A's spread (largest minus smallest round median: the noise of the box) and whether B's median
exceeds A's by no more than that spread.  Prints one JSON line; exit status 1 if a word differs or a shape exceeds the spread (such a
shape is then to be explained from the kernels' instruction streams, or the change behind it taken back).
--no-timing / --no-bits leave a half out."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ab_libs import load_once  # noqa: E402

RUNS = (0, 1, 7, 64)            # 0: the library's choice
F32 = np.float32


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def compare_bits(libs, torch):
    import compress_reference as C
    import filter_reference as Fr
    dev = torch.device("cuda", 0)

    def to_dev(v):
        return torch.from_numpy(np.ascontiguousarray(v, F32)).to(dev)

    def nan(*shape):
        return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)

    def ws(nbytes):
        return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)

    def compress(fa, c, run):
        """( out, gain ); run None: the host form"""
        if run is None:
            return fa.compress(c["x"], c["sr"], sidechain=c["side"], want_gain=True, **c["params"])
        ch, n = c["x"].shape
        side = c["x"] if c["side"] is None else c["side"]
        d_x = to_dev(c["x"])
        d_side = d_x if c["side"] is None else to_dev(side)
        d_out, d_gain = nan(ch, n), nan(n)
        params = {k: (v if np.isscalar(v) else to_dev(v)) for k, v in c["params"].items()}
        with fa.compress_run_forced(run):
            fa.compress_dev(d_x, ch, n, c["sr"], d_side, side.shape[0], side.shape[1], d_out, d_gain, ws(fa.compress_workspace_bytes(n)), **params)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_gain.cpu().numpy()

    def filt(fa, c, run):
        if run is None:
            return (fa.filter_1pole(c["x"], c["sr"], c["cutoff"], c["kind"], c["order"]),)
        ch, n = c["x"].shape
        d_out = nan(ch, n)
        cutoff = c["cutoff"] if np.isscalar(c["cutoff"]) else to_dev(c["cutoff"])
        with fa.filter_run_forced(run):
            fa.filter_1pole_dev(to_dev(c["x"]), ch, n, c["sr"], cutoff, c["kind"], c["order"], d_out, ws(fa.filter_1pole_workspace_bytes(ch, n)))
        torch.cuda.synchronize()
        return (d_out.cpu().numpy(),)

    res = {}
    for family, cases, call in (("compress", C.CASES, compress), ("filter_1pole", Fr.CASES, filt)):
        compared, differing = 0, []
        for c in cases:
            for run in (None,) + RUNS:
                got = {k: call(fa, c, run) for k, fa in libs.items()}
                for a, b in zip(got["A"], got["B"]):
                    compared += 1
                    if a.shape != b.shape or not np.array_equal(words(a), words(b)):
                        differing.append("%s %s" % (c["name"], "host" if run is None else "dev run %d" % run))
        res[family] = {"cases": len(cases), "forms": ["host"] + ["dev run %d" % r for r in RUNS], "arrays_compared": compared,
                       "bit_identical": not differing, "differing": differing}
    return res


def time_shapes(libs, torch, rounds, window_s, warmup, channels, seconds):
    dev = torch.device("cuda", 0)
    sr = 48000.0
    n, ch = int(seconds * sr) // 4 * 4, channels
    any_fa = libs["A"]
    amp = torch.where((torch.arange(n, device=dev) // 300) % 2 == 0, 0.5, 0.01)
    d_bursts = ((2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1) * amp).contiguous()
    d_noise = (2 * torch.rand((ch, n), dtype=torch.float32, device=dev) - 1).contiguous()
    t = torch.arange(n, dtype=torch.float32, device=dev) / n
    curves = dict(threshold=(-30.0 + 20.0 * t).contiguous(), ratio=(2.0 + 4.0 * t).contiguous(), attack=(0.001 + 0.02 * t).contiguous(),
                  release=(0.05 + 0.2 * t).contiguous(), knee_width=(6.0 * t).contiguous())
    constants = dict(threshold=-20.0, ratio=3.0, attack=0.005, release=0.1, knee_width=0.0)
    d_sweep = (200.0 * (8000.0 / 200.0) ** t).contiguous()
    # both builds write the same buffers (they never run at once): where a buffer lies in HBM is then no difference between them
    d_out, d_gain = torch.empty_like(d_noise), torch.empty(n, dtype=torch.float32, device=dev)
    d_cws = torch.empty(any_fa.compress_workspace_bytes(n), dtype=torch.uint8, device=dev)
    d_fws = torch.empty(any_fa.filter_1pole_workspace_bytes(ch, n), dtype=torch.uint8, device=dev)

    def comp(params):
        return lambda k: libs[k].compress_dev(d_bursts, ch, n, sr, d_bursts, ch, n, d_out, d_gain, d_cws, **params)

    def filt(cutoff, order):
        return lambda k: libs[k].filter_1pole_dev(d_noise, ch, n, sr, cutoff, libs[k].FILTER_BUTTERWORTH_LOW, order, d_out, d_fws)

    shapes = [("compress, constant parameters", comp(constants)), ("compress, per-frame parameters", comp(curves))]
    for cutoff_name, cutoff in (("constant", 1000.0), ("swept", d_sweep)):
        for order in (1, 2, 8):
            shapes.append(("filter_1pole low %d, %s cutoff" % (order, cutoff_name), filt(cutoff, order)))

    def round_median(fn, k):
        for _ in range(warmup):
            fn(k)
        torch.cuda.synchronize()
        times = []
        while sum(times) < window_s * 1e3 or len(times) < 5:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(k)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        return float(np.median(times))

    for _, fn in shapes:                                 # the device's clocks, every kernel loaded
        for k in libs:
            for _ in range(20):
                fn(k)
    torch.cuda.synchronize()
    meds = {name: {k: [] for k in libs} for name, _ in shapes}
    for r in range(rounds):
        for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
            for name, fn in shapes:
                meds[name][k].append(round_median(fn, k))
    out = []
    for name, _ in shapes:
        a, b = meds[name]["A"], meds[name]["B"]
        a_med, b_med, spread = float(np.median(a)), float(np.median(b)), max(a) - min(a)
        out.append({"shape": name, "A_ms": round(a_med, 5), "B_ms": round(b_med, 5), "A_spread_ms": round(spread, 5),
                    "B_minus_A_ms": round(b_med - a_med, 5), "within_A_spread": bool(b_med - a_med <= spread),
                    "A_round_medians_ms": [round(v, 5) for v in a], "B_round_medians_ms": [round(v, 5) for v in b]})
    return {"channels": ch, "frames": n, "rounds": rounds, "window_s": window_s, "shapes": out}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--a", default=os.path.join(ROOT, "flan_amd", "libflanhip_base.so"))
    ap.add_argument("--b", default=os.path.join(ROOT, "flan_amd", "libflanhip.so"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of timed calls per shape, build and round")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--no-bits", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    import torch
    libs = {"A": load_once("fa_a", args.a), "B": load_once("fa_b", args.b)}
    for fa in libs.values():
        fa.check(fa.lib.flanhip_set_device(0))
    res = {"A": os.path.relpath(args.a, ROOT), "B": os.path.relpath(args.b, ROOT)}
    ok = True
    if not args.no_bits:
        res["bits"] = compare_bits(libs, torch)
        ok = ok and all(v["bit_identical"] for v in res["bits"].values())
    if not args.no_timing:
        res["times"] = time_shapes(libs, torch, args.rounds, args.window, args.warmup, args.channels, args.seconds)
        ok = ok and all(s["within_A_spread"] for s in res["times"]["shapes"])
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
