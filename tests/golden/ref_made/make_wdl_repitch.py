#!/usr/bin/env python3
"""Vectors of Audio::repitch made by the reference's own WDL_Resampler (src/WDL/resample.cpp, compiled in place into a temporary
directory together with wdl_repitch_driver.cpp, which runs the block loop of Audio/AudioTemporal.cpp:251-296 around it).

    python tests/golden/ref_made/make_wdl_repitch.py        (needs /root/reference; run in the build container)

wdl_repitch.npz holds, per case k of `names`: x_k float32 [ch][n], inv_k the inverted and clamped factors (one per g input frames),
meta_k = (sample rate, g, quality, output frames, blocks), out_k float32 [ch][output frames], wanted_k and delivered_k int32 [blocks].
The cases are the smallest shapes at which each branch of the method can go wrong."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference/src"
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


def build(tmp):
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
    out = {"names": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for k, (name, sr, ch, n, g, curve, quality) in enumerate(CASES):
            rng = np.random.default_rng(1000 + k)
            x = (0.5 * rng.standard_normal((ch, n))).astype(F32)
            inv = invert(curve(n, g))
            y, wanted, delivered = run(L, x, sr, inv, g, quality)
            out["x_%d" % k], out["inv_%d" % k], out["out_%d" % k] = x, inv, y
            out["wanted_%d" % k], out["delivered_%d" % k] = wanted, delivered
            out["meta_%d" % k] = np.array([sr, g, quality, y.shape[1], wanted.size], np.float64)
            print("%-14s sr=%g ch=%d n=%d g=%d q=%d -> %d frames in %d blocks" % (name, sr, ch, n, g, quality, y.shape[1], wanted.size))
    path = os.path.join(HERE, "wdl_repitch.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
