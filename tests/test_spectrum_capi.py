"""The host-only half of the spectrum C ABI (include/flanhip.h, flanhip_spectrum_*) against tests/spectrum_reference.py, and every refusal the
entry points make before they ask for a device: runs on the CPU."""
import numpy as np
import pytest

import flan_amd as fa
import spectrum_reference as R

F32 = np.float32
INVALID, UNSUPPORTED = -1, -2


def test_error_codes_are_the_headers():
    assert (fa.ERR_INVALID_ARG, fa.ERR_UNSUPPORTED) == (INVALID, UNSUPPORTED)


@pytest.mark.parametrize("p,fp", [(6, 4), (6, 6), (10, 8), (13, 8), (14, 3), (20, 8), (22, 1)])
def test_bins(p, fp):
    harmonic, freq = fa.spectrum_bins(p, fp)
    want_h, want_f = R.bins(p, fp)
    assert harmonic.size == R.sizes(p)[2]
    assert np.array_equal(freq.view(np.uint32), want_f.view(np.uint32)) and np.array_equal(harmonic, want_h)


def test_bins_capacity_and_range():
    harmonic = np.full(10, -7, np.int32)
    assert fa.lib.flanhip_spectrum_bins(13, 8, fa._ptr(harmonic), None, 4) == 4097
    assert np.array_equal(harmonic[:4], R.bins(13, 8)[0][:4]) and np.all(harmonic[4:] == -7)
    assert fa.lib.flanhip_spectrum_bins(0, 8, None, None, 0) == 0 and fa.lib.flanhip_spectrum_bins(31, 8, None, None, 0) == 0


def test_num_harmonics():
    for fp in range(1, 23):
        assert fa.spectrum_num_harmonics(fp) == R.num_harmonics(fp)
    assert fa.spectrum_num_harmonics(8) == 189 and fa.spectrum_num_harmonics(-1) == 0


@pytest.mark.parametrize("seed", [0, 1, 4242, 2 ** 32 - 1])
def test_phases(seed):
    harmonic, _ = R.bins(13, 8)
    theta = fa.spectrum_phases(seed, harmonic)
    assert np.array_equal(theta.view(np.uint32), R.phases(seed, harmonic).view(np.uint32))
    assert np.all(theta[harmonic == 0] == 0) and np.all(theta < R.PI2) and np.all(theta >= 0)
    # ascending bin order: dropping a bin's harmonic shifts every later draw down by one bin
    h2 = harmonic.copy()
    first = int(np.flatnonzero(h2)[0])
    h2[first] = 0
    t2 = fa.spectrum_phases(seed, h2)
    on, on2 = np.flatnonzero(harmonic), np.flatnonzero(h2)
    assert np.array_equal(theta[on][:-1], t2[on2])


def test_jump():
    for p in (6, 13, 20, 22):
        for ch in (1, 2, 3, 5, 7):
            assert [fa.spectrum_jump(c, ch, p) for c in range(ch)] == [R.jump(c, ch, p) for c in range(ch)]
    assert fa.spectrum_jump(3, 3, 13) == 0 and fa.spectrum_jump(0, 0, 13) == 0


@pytest.mark.parametrize("fundamental,freq", [(256.0, [220.0]), (256.0, np.linspace(110, 880, 4800)), (8.0, [20.0]), (256.0, [1000.0])])
def test_synth_plan(fundamental, freq):
    plan = fa.spectrum_synth_plan(4800, fundamental, 48, freq)
    want = R.synth_plan(4800, fundamental, 48, freq)
    for name in ("offset", "fracpos", "ratio", "filtpos", "oversize", "ideal", "first_out", "num_out", "wanted", "in_start"):
        assert np.array_equal(plan[name], np.array([b[name] for b in want], plan[name].dtype)), name
    # the wavetable plan at sr = fundamental * N is the same plan
    other = fa.wavetable_synth_plan(4800, fundamental * 8192, 8192, 48, freq)
    for name in plan:
        assert np.array_equal(plan[name], other[name]), name


def rc_table(mag, theta, p, table):
    return fa.lib.flanhip_spectrum_table(None if mag is None else fa._ptr(mag), None if theta is None else fa._ptr(theta), p,
                                         None if table is None else fa._ptr(table), None)


def test_table_refusals():
    for p in (5, 23, 0, -1):
        B = (1 << max(p - 1, 0)) + 1
        z = np.zeros(B, F32)
        assert rc_table(z, z, p, np.zeros(1 << max(p, 0), F32)) == UNSUPPORTED, p
        assert fa.spectrum_table_workspace_bytes(p) == 0
        assert fa.lib.flanhip_spectrum_table_dev(None, None, p, None, None, None) == UNSUPPORTED
    z, t = np.zeros(33, F32), np.zeros(64, F32)
    assert rc_table(None, z, 6, t) == INVALID and rc_table(z, None, 6, t) == INVALID and rc_table(z, z, 6, None) == INVALID
    assert "null buffer" in fa.last_error()
    assert fa.lib.flanhip_spectrum_table_dev(fa._ptr(z), fa._ptr(z), 6, fa._ptr(t), None, None) == INVALID          # null workspace
    assert [fa.spectrum_table_workspace_bytes(p) for p in (6, 13, 14, 22)] == [8 << 5, 8 << 12, 8 << 13, 8 << 21]


def rc_synth(table, p, rate_out, ch, frames, g, freq, out):
    f = None if freq is None else np.ascontiguousarray(freq, F32)
    return fa.lib.flanhip_spectrum_synth(None if table is None else fa._ptr(table), p, rate_out, ch, frames, g, None if f is None else fa._ptr(f),
                                         0 if f is None else f.size, None if out is None else fa._ptr(out), None)


def test_synth_refusals():
    table, out = np.zeros(64, F32), np.zeros((2, 100), F32)
    ok = dict(table=table, p=6, rate_out=16.0, ch=2, frames=100, g=10, freq=[100.0], out=out)

    def rc(**kw):
        return rc_synth(**dict(ok, **kw))
    assert rc(p=5) == UNSUPPORTED and rc(p=23) == UNSUPPORTED
    assert rc(table=None) == INVALID and rc(out=None) == INVALID and rc(freq=None) == INVALID
    assert rc(g=0) == INVALID and "granularity" in fa.last_error()
    assert rc(frames=0) == INVALID and rc(ch=0) == INVALID and rc(rate_out=0.0) == INVALID and rc(rate_out=float("nan")) == INVALID
    assert rc(freq=[float("inf")]) == INVALID
    # a ratio above 34 after the first block: the refusal of the wavetable plan, unchanged
    assert rc(freq=np.r_[np.full(50, 100.0), np.full(50, 1000.0)]) == UNSUPPORTED and "ratio above 34" in fa.last_error()
    assert fa.spectrum_synth_workspace_bytes(6, 16.0, 2, 100, 0, [100.0]) == 0
    assert fa.spectrum_synth_workspace_bytes(5, 16.0, 2, 100, 10, [100.0]) == 0
    assert fa.spectrum_synth_workspace_bytes(6, 16.0, 2, 100, 10, [100.0]) > 0
    assert fa.lib.flanhip_spectrum_synth_plan(100, 16.0, 0, fa._ptr(np.zeros(1, F32)), 1, 0, *([None] * 10)) == INVALID


def rc_whole(mag, theta, p, fp, ch, frames, g, freq, out):
    f = None if freq is None else np.ascontiguousarray(freq, F32)
    return fa.lib.flanhip_audio_synthesize_spectrum(None if mag is None else fa._ptr(mag), None if theta is None else fa._ptr(theta), p, fp, ch, frames, g,
                                                    None if f is None else fa._ptr(f), 0 if f is None else f.size, None if out is None else fa._ptr(out),
                                                    None)


def test_whole_call_refusals():
    z, out = np.zeros(33, F32), np.zeros((2, 100), F32)
    ok = dict(mag=z, theta=z, p=6, fp=4, ch=2, frames=100, g=10, freq=[100.0], out=out)

    def rc(**kw):
        return rc_whole(**dict(ok, **kw))
    assert rc(p=5) == UNSUPPORTED and rc(p=23, fp=8) == UNSUPPORTED
    assert rc(fp=0) == INVALID and rc(fp=7) == INVALID                            # AudioSynthesis.cpp:164-166
    assert rc(g=0) == INVALID and "granularity" in fa.last_error()
    assert rc(mag=None) == INVALID and rc(theta=None) == INVALID and rc(out=None) == INVALID and rc(freq=None) == INVALID
    assert rc(frames=0) == INVALID and rc(ch=0) == INVALID
    assert fa.audio_synthesize_spectrum_workspace_bytes(6, 4, 2, 100, 0, [100.0]) == 0
    assert fa.audio_synthesize_spectrum_workspace_bytes(23, 8, 2, 100, 10, [100.0]) == 0
    ws = fa.audio_synthesize_spectrum_workspace_bytes(13, 8, 2, 4800, 48, [220.0])
    assert ws >= 4 * 8192 + fa.spectrum_table_workspace_bytes(13) + fa.audio_set_volume_workspace_bytes(2, 4800)
