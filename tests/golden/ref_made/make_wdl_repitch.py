#!/usr/bin/env python3
"""Vectors of Audio::repitch made by the reference's own WDL_Resampler (src/WDL/resample.cpp, compiled in place into a temporary
directory together with wdl_repitch_driver.cpp, which runs the block loop of Audio/AudioTemporal.cpp:251-296 around it).

    FLAN_REFERENCE_SRC=<the reference's src directory> python tests/golden/ref_made/make_wdl_repitch.py [runs]

Without an argument it writes wdl_repitch.npz from CASES; with `runs`, wdl_repitch_runs.npz from RUN_CASES, the shapes that hold the run
planner of the sinc launch (the window cut, the global-memory taps, the channel groups: DESIGN.md 4.13).  Either file holds, per case k
of `names`: x_k float32 [ch][n], inv_k the inverted and clamped factors (one per g input frames),
meta_k = (sample rate, g, quality, output frames, blocks), out_k float32 [ch][output frames], wanted_k and delivered_k int32 [blocks].
The cases are the smallest shapes at which each branch of the method can go wrong."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("FLAN_REFERENCE_SRC", "")
SINC, LINEAR, UNINTERPOLATED = 0, 1, 2
F32 = np.float32


def invert(factors):
    """AudioTemporal.cpp:246-249 in fp32: clamp( 1.0f / v, 1.0f / 1000.0f, 1000.0f )"""
    with np.errstate(divide="ignore"):
        inv = F32(1.0) / np.asarray(factors, F32)
    return np.clip(inv, F32(1.0) / F32(1000.0), F32(1000.0)).astype(F32)


def count_of(n, g):
    return int(np.ceil(F32(n) / F32(g)))                      # :245, ceil( N / float( g ) )


def constant(v):
    return lambda n, g: np.full(count_of(n, g), v, F32)


def sweep(a, b):
    def f(n, g):
        c = count_of(n, g)
        return (a + (b - a) * np.arange(c) / max(c - 1, 1)).astype(F32)
    return f


def step(n, g):
    c = count_of(n, g)
    v = np.ones(c, F32)
    v[c // 3:2 * c // 3] = 1.5
    return v


# ( name, sample rate, channels, n, g, factor curve, quality )
CASES = [
    ("n1", 48000.0, 1, 1, 48, constant(1.5), SINC),
    ("n20", 48000.0, 1, 20, 48, constant(0.7), SINC),                   # shorter than the 31-sample prelude
    ("one_ideal1", 48000.0, 1, 1000, 48, constant(1.0), SINC),          # ideal, oversize 1
    ("half_ideal2", 48000.0, 2, 1000, 48, constant(0.5), SINC),         # ideal, oversize 2
    ("p8_gcd5", 48000.0, 3, 1000, 48, constant(0.8), SINC),             # ideal through the GCD, oversize 5
    ("two_ideal_lp", 48000.0, 1, 1000, 48, constant(2.0), SINC),        # ideal with a low-pass
    ("up1p5", 48000.0, 2, 1000, 48, constant(1.5), SINC),               # not ideal, ratio > 1
    ("down0p7", 48000.0, 3, 1000, 48, constant(0.7), SINC),             # not ideal, ratio < 1
    ("g1_up", 48000.0, 1, 300, 1, constant(1.5), SINC),
    ("g1_down", 48000.0, 2, 300, 1, constant(0.7), SINC),
    ("g5000", 48000.0, 1, 1000, 5000, constant(1.5), SINC),             # g > n: one block
    ("sweep", 48000.0, 1, 4000, 48, sweep(0.5, 2.0), SINC),             # a table per block, crossing ratio 1
    ("zero", 48000.0, 1, 50, 48, constant(0.0), SINC),                  # 1 / 0 = inf: the upper clamp, 1000 x longer
    ("negative", 48000.0, 1, 50, 48, constant(-2.0), SINC),             # the lower clamp
    ("tiny", 48000.0, 1, 50, 48, constant(1e-6), SINC),                 # the upper clamp
    ("step", 48000.0, 1, 1000, 48, step, SINC),                         # ideal, not ideal, ideal again: the fracpos quantisation
    ("cd_0p9", 44100.0, 1, 1000, 44, constant(0.9), SINC),
    ("u_up1p5", 48000.0, 2, 1000, 48, constant(1.5), UNINTERPOLATED),
    ("u_down0p7", 48000.0, 3, 1000, 48, constant(0.7), UNINTERPOLATED),
    ("u_sweep", 48000.0, 1, 4000, 48, sweep(0.5, 2.0), UNINTERPOLATED),
    ("u_step", 48000.0, 1, 1000, 48, step, UNINTERPOLATED),
]


def thirds(a, b):
    def f(n, g):
        c = count_of(n, g)
        v = np.full(c, a, F32)
        v[c // 3:2 * c // 3] = b
        return v
    return f


# The same columns, random seeds 1100 + k.  What each shape must reach is asserted from the exported run table by
# tests/test_gpu_repitch.py (RUN_PATHS), so a retuning of the planner's limits fails there instead of un-covering the path.
RUN_CASES = [
    ("global_3p9", 48000.0, 1, 13000, 1600, constant(3.9), SINC),       # a block's own window is past the staging buffer: taps from global memory, offset > 0
    ("global_ideal4", 48000.0, 2, 13000, 1600, constant(4.0), SINC),    # the same through the one-sum (ideal) path, low-pass table
    ("window_cut", 48000.0, 2, 8000, 48, constant(3.9), SINC),          # multi-block runs closed by the window, not by the block cap
    ("window_cut_g1", 48000.0, 1, 7000, 1, constant(3.9), SINC),        # the same at g = 1: more than 1500 blocks in a run
    ("step_3p9", 48000.0, 2, 12000, 48, thirds(1.0, 3.9), SINC),        # table cuts and block-cap cuts in one call, ideal and not ideal blocks
    ("groups_sweep", 48000.0, 13, 2000, 48, sweep(0.5, 2.0), SINC),     # a table per block: several channels per workgroup, a ragged last group
    ("groups_small", 48000.0, 5, 200, 48, constant(1.0), SINC),         # one short run: channel groups of 2, 2 and 1
]


def build(tmp):
    assert REFERENCE, "set FLAN_REFERENCE_SRC to the reference's src directory"
    lib = os.path.join(tmp, "libwdlrepitch.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I" + REFERENCE,
                    os.path.join(HERE, "wdl_repitch_driver.cpp"), os.path.join(REFERENCE, "WDL", "resample.cpp"), "-o", lib], check=True)
    L = C.CDLL(lib)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.wdl_repitch_out_frames.restype = C.c_int64
    L.wdl_repitch_out_frames.argtypes = [f32p, C.c_int64, C.c_int]
    L.wdl_repitch.restype = C.c_int64
    L.wdl_repitch.argtypes = [f32p, C.c_int, C.c_int, C.c_float, f32p, C.c_int, C.c_int, f32p, C.c_int, i32p, i32p, C.c_int64]
    return L


def run(L, x, sr, inv, g, quality):
    ch, n = x.shape
    nout = int(L.wdl_repitch_out_frames(inv, inv.size, g))
    out = np.zeros((ch, nout), F32)
    cap = 1 << 20
    wanted, delivered = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    blocks = int(L.wdl_repitch(np.ascontiguousarray(x).reshape(-1), ch, n, sr, inv, g, quality, out.reshape(-1), nout, wanted, delivered, cap))
    assert blocks <= cap
    return out, wanted[:blocks].copy(), delivered[:blocks].copy()


def main():
    runs = sys.argv[1:] == ["runs"]
    assert runs or not sys.argv[1:], "usage: make_wdl_repitch.py [runs]"
    cases, seed0, target = (RUN_CASES, 1100, "wdl_repitch_runs.npz") if runs else (CASES, 1000, "wdl_repitch.npz")
    out = {"names": np.array([c[0] for c in cases])}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for k, (name, sr, ch, n, g, curve, quality) in enumerate(cases):
            rng = np.random.default_rng(seed0 + k)
            x = (0.5 * rng.standard_normal((ch, n))).astype(F32)
            inv = invert(curve(n, g))
            y, wanted, delivered = run(L, x, sr, inv, g, quality)
            out["x_%d" % k], out["inv_%d" % k], out["out_%d" % k] = x, inv, y
            out["wanted_%d" % k], out["delivered_%d" % k] = wanted, delivered
            out["meta_%d" % k] = np.array([sr, g, quality, y.shape[1], wanted.size], np.float64)
            print("%-14s sr=%g ch=%d n=%d g=%d q=%d -> %d frames in %d blocks" % (name, sr, ch, n, g, quality, y.shape[1], wanted.size))
    path = os.path.join(HERE, target)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
