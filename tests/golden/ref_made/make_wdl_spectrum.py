#!/usr/bin/env python3
"""Vectors of Audio::synthesize_spectrum's loop made by the reference's own WDL_Resampler (src/WDL/resample.cpp, compiled in place into a
temporary directory together with wdl_spectrum_driver.cpp, which runs the block loop of Audio/AudioSynthesis.cpp:230-263 around it).

    FLAN_REFERENCE_SRC=<the reference's src directory> python tests/golden/ref_made/make_wdl_spectrum.py

wdl_spectrum.npz holds, per case k of `names`: table_k float32 [2^p] (tests/spectrum_reference.golden_table), freq_k float32 [frames] (the
frequency at every output frame: a block reads that of its first frame), meta_k = (p, fundamental, channels, g, output frames, blocks),
out_k float32 [ch][frames], wanted_k and delivered_k int32 [blocks]."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import spectrum_reference as R          # noqa: E402

F32 = np.float32
CHANNELS, G, FRAMES = 3, 48, 4800


def const(v):
    return lambda n: np.full(n, v, F32)


def sweep(a, b):
    return lambda n: (a + (b - a) * np.arange(n) / max(n - 1, 1)).astype(F32)


# ( name, p, fundamental_power, freq curve )
CASES = [
    ("p13_f220", 13, 8, const(220.0)),               # ratio 0.859, oversize 64
    ("p13_f256", 13, 8, const(256.0)),               # ratio 1, oversize 1
    ("p14_f1000", 14, 8, const(1000.0)),             # ratio 3.9, a low-pass table; the stream wraps the period
    ("p13_sweep", 13, 8, sweep(110.0, 880.0)),       # non-ideal ratios, a table per block; wraps
    ("p14_fund8_f20", 14, 3, const(20.0)),           # ratio 2.5
]


def build(tmp):
    reference = os.environ["FLAN_REFERENCE_SRC"]
    lib = os.path.join(tmp, "libwdlspectrum.so")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I" + reference,
                    os.path.join(HERE, "wdl_spectrum_driver.cpp"), os.path.join(reference, "WDL", "resample.cpp"), "-o", lib], check=True)
    L = C.CDLL(lib)
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C_CONTIGUOUS")
    L.wdl_spectrum.restype = C.c_int64
    L.wdl_spectrum.argtypes = [f32p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, f32p, f32p, i32p, i32p, C.c_int64]
    return L


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        for k, (name, p, fp, fcurve) in enumerate(CASES):
            table = R.golden_table(p)
            freq = fcurve(FRAMES)
            y = np.zeros((CHANNELS, FRAMES), F32)
            cap = 1 << 16
            wanted, delivered = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
            blocks = int(L.wdl_spectrum(table, 1 << p, float(2 ** fp), CHANNELS, FRAMES, G, freq, y.reshape(-1), wanted, delivered, cap))
            assert 0 < blocks <= cap
            out["table_%d" % k], out["freq_%d" % k], out["out_%d" % k] = table, freq, y
            out["wanted_%d" % k], out["delivered_%d" % k] = wanted[:blocks].copy(), delivered[:blocks].copy()
            out["meta_%d" % k] = np.array([p, 2 ** fp, CHANNELS, G, FRAMES, blocks], np.float64)
            print("%-16s p=%d fundamental=%d -> %d blocks, %d input samples, delivered %d ... %d" % (
                name, p, 2 ** fp, blocks, int(wanted[:blocks].sum()), delivered[:blocks].min(), delivered[:blocks].max()))
    path = os.path.join(HERE, "wdl_spectrum.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
