#!/usr/bin/env python3
"""Vectors of Wavetable::synthesize made by the reference's own WDL_Resampler (src/WDL/resample.cpp, compiled in place into a temporary
directory together with wdl_wavetable_driver.cpp, which runs the block loop of Wavetable.cpp:293-330 around it).

    FLAN_REFERENCE_SRC=<the reference's src directory> python tests/golden/ref_made/make_wdl_wavetable.py [runs]

Without an argument it writes wdl_wavetable.npz from CASES; with `runs`, wdl_wavetable_runs.npz from RUN_CASES, the shapes that hold the run
planner of the synthesis launch (blocks cut into pieces, channel groups: DESIGN.md 4.23).  Either file holds, per case k of `names`:
table_k float32 [ch][slots * W], freq_k float32 [frames] and index_k float32 [ch][frames]
(the frequency and the table index at every output frame: a block reads those of its first frame), meta_k = (sample rate, W, g, output
frames, smooth, blocks), out_k float32 [ch][frames], wanted_k and delivered_k int32 [blocks].  The table indices come from
tests/wavetable_reference.table_index over starts_k (one row per channel, padded with -1) and ratio_k float32 [frames]."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import wavetable_reference as R          # noqa: E402

F32 = np.float32
SR = 48000.0
SOURCE_FRAMES = 1000
STARTS = [[0, 210, 433, 640, 870], [5, 300, 610]]          # two channels with different waveform_starts: 5 slots, the second fills 2


def const(v):
    return lambda n: np.full(n, v, F32)


def sweep(a, b):
    return lambda n: (a + (b - a) * np.arange(n) / max(n - 1, 1)).astype(F32)


# ( name, W, g, frames, freq curve, ratio curve, smooth )
CASES = [
    ("f750_ideal1", 64, 48, 2400, const(750.0), const(0.37), True),
    ("f1500_ideal_lp", 64, 48, 2400, const(1500.0), const(0.37), True),
    ("f375_ideal2", 64, 48, 2400, const(375.0), const(0.37), True),
    ("f1027p5", 64, 48, 2400, const(1027.5), const(0.37), True),
    ("f100", 64, 48, 2400, const(100.0), sweep(0.0, 1.0), True),             # 6 input samples per block: a tap window spans many blends
    ("fsweep", 64, 48, 2400, sweep(200.0, 3000.0), const(0.37), True),       # a table per block, crossing ratio 1
    ("f0", 64, 48, 2400, const(0.0), const(0.37), True),                     # the 1 Hz clamp
    ("fneg5", 64, 48, 2400, const(-5.0), sweep(0.0, 1.0), True),
    ("rsweep", 64, 48, 2400, const(1027.5), sweep(0.0, 1.0), True),
    ("rneg", 64, 48, 2400, const(1027.5), const(-0.5), True),                # the clamps of the table index
    ("rbig", 64, 48, 2400, const(1027.5), const(1.5), True),
    ("unsmooth", 64, 48, 2400, const(1027.5), sweep(0.0, 1.0), False),
    ("plus17", 64, 48, 2417, const(1027.5), sweep(0.0, 1.0), True),          # the capped last block
    ("frames20", 64, 48, 20, const(1027.5), const(0.37), True),              # shorter than g
    ("w2048", 2048, 48, 2400, const(220.0), sweep(0.0, 1.0), True),
]


# The cases of the run planner: W = 64, smooth, the ratio swept 0 -> 1, random tables of 3 slots.  ( name, channels, g, frames, freq curve ).
# What each shape must reach is asserted from the exported run table by tests/test_gpu_wavetable.py (RUN_PATHS).
RUN_W, RUN_SLOTS = 64, 3
RUN_CASES = [
    ("piece_window", 2, 480, 1500, const(9803.7)),                # ratio 13.07, not ideal (9800 Hz is, through the GCD): every full block's window is past the staging buffer
    ("piece_ratio32", 1, 480, 1200, const(24000.0)),              # ratio 32 (ideal, low-pass), the largest below the refusal: 3 pieces a block
    ("piece_outputs_and_window", 2, 4800, 6000, const(2227.2)),   # ratio 2.9696: 2047 steps span 6078 or 6079 samples, so one block is cut at 2048 outputs and by the window
    ("groups", 7, 100, 1200, sweep(225.0, 2475.0)),               # a table per block: 4 channels per workgroup, groups of 4 and 3
]


def run_starts(ch):
    """3 starts per channel, different in every channel, inside the 1000 source frames"""
    return [[0, 300 + 20 * c, 700 + 30 * c] for c in range(ch)]


def make_table(W, seed):
    """5 slots of smooth random waveforms; the slots a channel does not fill stay 0, as resample_waveforms leaves them"""
    rng = np.random.default_rng(seed)
    slots = max(len(s) for s in STARTS)
    table = np.zeros((len(STARTS), slots * W), F32)
    t = np.arange(W) / W
    for c, s in enumerate(STARTS):
        for w in range(len(s) - 1):
            a = rng.standard_normal(4) * [0.5, 0.3, 0.15, 0.05]
            ph = rng.uniform(0, 2 * np.pi, 4)
            table[c, w * W:(w + 1) * W] = sum(a[h] * np.sin(2 * np.pi * (h + 1) * t + ph[h]) for h in range(4)).astype(F32)
    return table


def build(tmp):
    reference = os.environ["FLAN_REFERENCE_SRC"]
    lib = os.path.join(tmp, "libwdlwavetable.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I" + reference,
                    os.path.join(HERE, "wdl_wavetable_driver.cpp"), os.path.join(reference, "WDL", "resample.cpp"), "-o", lib], check=True)
    L = C.CDLL(lib)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.wdl_wavetable.restype = C.c_int64
    L.wdl_wavetable.argtypes = [f32p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, f32p, f32p, C.c_int, f32p, i32p, i32p, C.c_int64]
    return L


def main():
    runs = sys.argv[1:] == ["runs"]
    assert runs or not sys.argv[1:], "usage: make_wdl_wavetable.py [runs]"
    if runs:
        cases = [(name, RUN_W, g, frames, fcurve, sweep(0.0, 1.0), True, run_starts(ch)) for name, ch, g, frames, fcurve in RUN_CASES]
    else:
        cases = [c + (STARTS,) for c in CASES]
    out = {"names": np.array([c[0] for c in cases])}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for k, (name, W, g, frames, fcurve, rcurve, smooth, case_starts) in enumerate(cases):
            if runs:
                table = (0.5 * np.random.default_rng(2100 + k).standard_normal((len(case_starts), RUN_SLOTS * W))).astype(F32)
            else:
                table = make_table(W, 2000 + k)
            ch, slots = table.shape[0], table.shape[1] // W
            freq, ratio = fcurve(frames), rcurve(frames)
            index = np.array([[R.table_index(s, SOURCE_FRAMES, r) for r in ratio] for s in case_starts], F32)
            y = np.zeros((ch, frames), F32)
            cap = 1 << 16
            wanted, delivered = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            blocks = int(L.wdl_wavetable(table.reshape(-1), ch, slots, W, SR, frames, g, freq, index.reshape(-1), int(smooth), y.reshape(-1),
                                         wanted, delivered, cap))
            assert 0 < blocks <= cap
            assert int(delivered[:blocks].sum()) == frames, "the reference's resampler did not deliver every frame"
            starts = np.full((ch, slots), -1, np.int32)
            for c, s in enumerate(case_starts):
                starts[c, :len(s)] = s
            out["table_%d" % k], out["freq_%d" % k], out["ratio_%d" % k], out["index_%d" % k], out["out_%d" % k] = table, freq, ratio, index, y
            out["starts_%d" % k] = starts
            out["wanted_%d" % k], out["delivered_%d" % k] = wanted[:blocks].copy(), delivered[:blocks].copy()
            out["meta_%d" % k] = np.array([SR, W, g, frames, int(smooth), blocks], np.float64)
            print("%-16s W=%d g=%d frames=%d -> %d blocks, delivered %d ... %d" % (name, W, g, frames, blocks, delivered[:blocks].min(), delivered[:blocks].max()))
    path = os.path.join(HERE, "wdl_wavetable_runs.npz" if runs else "wdl_wavetable.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
