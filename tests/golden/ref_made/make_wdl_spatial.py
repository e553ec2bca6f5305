#!/usr/bin/env python3
"""Vectors of head_itd (Audio/AudioSpatial.cpp:135-221, the heart of Audio::stereo_spatialize) made by the reference's own
WDL_Resampler (src/WDL/resample.cpp, compiled in place into a temporary directory together with wdl_spatial_driver.cpp, which runs the
loop of :159-218 around it).

    python tests/golden/ref_made/make_wdl_spatial.py        (needs /root/reference; run in the build container)

A case is a source path: float32 positions per frame, run through the speed limiter of tests/spatial_reference.py and taken relative to
the left ear of a head 0.18 m wide; the driver gets the distances at frames 0, 32, 64, ...  wdl_spatial.npz holds, per case k of `names`:
x_k float32 [n] (noise), dist_k float64 [ceil( n / 32 )], stretches_k float64 (the driver's), out_k float32 [output frames],
delivered_k int32 [blocks] (what ResampleOut returned per block), meta_k = (sample rate, output frames, blocks).
The cases are the smallest shapes at which each branch of the method can go wrong."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import spatial_reference as S                                  # noqa: E402  (the limiter and the ear geometry only)

REFERENCE = "/root/reference/src"
F32 = np.float32


def line(p0, velocity):
    """a straight path from p0 at `velocity` metres per second"""
    def f(n, sr):
        t = np.arange(n)[:, None] / sr
        return (np.asarray(p0)[None, :] + t * np.asarray(velocity)[None, :]).astype(F32)
    return f


def orbit(radius, hz):
    def f(n, sr):
        a = 2 * np.pi * hz * np.arange(n) / sr
        return np.stack([radius * np.cos(a), radius * np.sin(a)], 1).astype(F32)
    return f


def walk(seed, step):
    def f(n, sr):
        rng = np.random.default_rng(seed)
        return (np.array([1.5, 0.5]) + np.cumsum(step * rng.standard_normal((n, 2)), 0)).astype(F32)
    return f


def still_in_the_middle(n, sr):
    p = line((3.0, 1.0), (-40.0, 5.0))(n, sr)
    p[n // 3:2 * n // 3] = p[n // 3]                              # the same float pair for a third of the frames: stretch exactly 1
    return p


def jump(p0, p1, at):
    def f(n, sr):
        p = np.tile(np.asarray(p0, F32), (n, 1))
        p[at:] = np.asarray(p1, F32)
        return p
    return f


# ( name, sample rate, n, path )
CASES = [
    ("n1", 48000.0, 1, line((2.0, 1.0), (3.0, 0.0))),
    ("n20", 48000.0, 20, line((2.0, 1.0), (3.0, 0.0))),
    ("n32", 48000.0, 32, line((2.0, 1.0), (3.0, 0.0))),                 # one block, no output frames
    ("n33", 48000.0, 33, line((2.0, 1.0), (30.0, 0.0))),                # two blocks
    ("n64", 48000.0, 64, line((2.0, 1.0), (-30.0, 0.0))),
    ("n100", 48000.0, 100, line((2.0, 1.0), (30.0, 10.0))),             # the prelude and the dropped tail
    ("orbit_1000", 48000.0, 1000, orbit(2.0, 40.0)),                    # the general path: ratio on both sides of 1
    ("walk_4000", 48000.0, 4000, walk(7, 2e-4)),
    ("walk_cd", 44100.0, 1000, walk(8, 2e-4)),
    ("receding", 48000.0, 2000, line((1.0, 0.0), (30.0, 0.0))),         # ratio < 1: one table
    ("approaching", 48000.0, 2000, line((50.0, 0.0), (-30.0, 0.0))),    # ratio > 1: a table per block
    ("flyby", 48000.0, 4000, line((-12.0, 2.0), (300.0, 0.0))),         # crosses ratio 1
    ("still", 48000.0, 2000, still_in_the_middle),                      # ratio exactly 1 in the middle: ideal, oversize 1, fracpos rounded
    ("jump_away", 48000.0, 80, jump((1.0, 0.0), (100.0, 0.0), 32)),     # the limiter makes it 342 m/s: stretch near 343, thousands of outputs a block
    ("jump_near", 48000.0, 400, jump((100.0, 0.0), (1.0, 0.0), 64)),    # approaching at 342 m/s: ratio near 2
    ("far", 48000.0, 1000, line((343.0, 0.0), (0.0, 5.0))),             # one second of sound travel: a long silent tail
]


def build(tmp):
    lib = os.path.join(tmp, "libwdlspatial.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I" + REFERENCE,
                    os.path.join(HERE, "wdl_spatial_driver.cpp"), os.path.join(REFERENCE, "WDL", "resample.cpp"), "-o", lib], check=True)
    L = C.CDLL(lib)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.wdl_spatial_out_frames.restype = C.c_int
    L.wdl_spatial_out_frames.argtypes = [C.c_int, C.c_float, f64p, C.c_int, f64p]
    L.wdl_spatial_itd.restype = C.c_int
    L.wdl_spatial_itd.argtypes = [f32p, C.c_int, C.c_float, f64p, C.c_int, f32p, C.c_int, i32p]
    return L


def run(L, x, sr, dist):
    stretches = np.zeros(dist.size, np.float64)
    nout = int(L.wdl_spatial_out_frames(x.size, sr, dist, dist.size, stretches))
    assert nout >= 0
    out = np.zeros(max(nout, 1), F32)
    delivered = np.zeros(dist.size, np.int32)
    blocks = int(L.wdl_spatial_itd(x, x.size, sr, stretches, dist.size, out, nout, delivered))
    assert blocks == dist.size
    return stretches, out[:nout].copy(), delivered


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for k, (name, sr, n, path) in enumerate(CASES):
            rng = np.random.default_rng(2000 + k)
            x = (0.5 * rng.standard_normal(n)).astype(F32)
            ps = S.limit_positions(path(n, sr), np.finfo(F32).max, sr)
            dist = np.ascontiguousarray(S.mag(S.relative(ps, 0.18, S.LEFT)[::S.G]))
            stretches, y, delivered = run(L, x, sr, dist)
            out["x_%d" % k], out["dist_%d" % k], out["stretches_%d" % k] = x, dist, stretches
            out["out_%d" % k], out["delivered_%d" % k] = y, delivered
            out["meta_%d" % k] = np.array([sr, y.size, delivered.size], np.float64)
            print("%-12s sr=%g n=%d -> %d frames, %d blocks delivering %d (most in one: %d), stretch %.4f ... %.4f"
                  % (name, sr, n, y.size, delivered.size, delivered.sum(), delivered.max(), stretches.min(), stretches.max()))
    path = os.path.join(HERE, "wdl_spatial.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


def time_driver(seconds):
    """--time SECONDS: the driver's head_itd (one ear, one CPU core of the machine this runs on) on the motions of tools/bench_spatial.py"""
    import time
    sr = 48000.0
    n = int(seconds * sr)
    x = (0.5 * np.random.default_rng(1).standard_normal(n)).astype(F32)
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for name, path in (("slow orbit", orbit(2.0, 0.5)), ("fly-by", line((-30.0 * seconds / 2, 2.0), (30.0, 0.0)))):
            dist = np.ascontiguousarray(S.mag(S.relative(path(n, sr).astype(np.float64), 0.18, S.LEFT)[::S.G]))
            times = []
            for _ in range(3):
                t0 = time.perf_counter()
                _, y, delivered = run(L, x, sr, dist)
                times.append((time.perf_counter() - t0) * 1e3)
            print("%-10s %d frames -> %d, %d blocks: the reference's loop for ONE ear %.1f ms (median of 3)" % (name, n, y.size, delivered.size, float(np.median(times))))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--time":
        time_driver(float(sys.argv[2]))
    else:
        main()
