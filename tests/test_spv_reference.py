"""The numpy restatement of the sliding-DFT vocoder (tests/spv_reference.py) against a literal scalar transcription of the reference's
loops (Conversions/AudioSPV.cpp:27-108) on tiny inputs, bit for bit, and against the fp64 truth of DESIGN.md 4.11's identity."""
import os

import numpy as np
import pytest

import oracle_lib as O
import spv_reference as R

F32 = np.float32
needs_ref = pytest.mark.skipif(not os.path.exists(O._REF), reason="oracle/_ref (the reference's phase_vocoder) is not built")


def scalar_spectra(x, N):
    """AudioSPV.cpp:45-92 one value at a time: float32 scalars, each complex operation spelled out as the C++ evaluates it."""
    n = len(x)
    L = 2 * N
    Tr, Ti = R.twiddles(N)

    def fid(f, b):
        k = (f * b) % L
        return Tr[k], Ti[k]

    d = [F32(x[f]) - (F32(x[f - L]) if f - L >= 0 else F32(0)) for f in range(n)]
    S = [[(F32(0), F32(0))] * N for _ in range(n)]
    for b in range(N):
        S[0][b] = (F32(d[0]), F32(0))
        for f in range(1, n):
            tr, ti = fid(f, b)
            pr, pi = F32(d[f] * tr), F32(d[f] * ti)
            S[f][b] = (F32(S[f - 1][b][0] + pr), F32(S[f - 1][b][1] + pi))
    out = np.zeros((n, N, 2), F32)
    for f in range(n):
        F = []
        for b in range(N):
            sr_, si_ = S[f][b]
            tr, ti = fid(f + 1, b)
            cr, ci = tr, F32(-ti)
            F.append((F32(F32(sr_ * cr) - F32(si_ * ci)), F32(F32(sr_ * ci) + F32(si_ * cr))))
        for b in range(N):
            a = (F32(F[b][0] + F[b][0]), F32(F[b][1] + F[b][1]))
            if b == 0:
                bb = (F32(F[1][0] * F32(2)), F32(0))
            elif b == N - 1:
                bb = (F32(F[N - 2][0] * F32(2)), F32(0))
            else:
                bb = (F32(F[b - 1][0] + F[b + 1][0]), F32(F[b - 1][1] + F[b + 1][1]))
            cv = (F32(F32(0.25) * F32(a[0] - bb[0])), F32(F32(0.25) * F32(a[1] - bb[1])))
            out[f, b] = (F32(cv[0] / F32(L)), F32(cv[1] / F32(L)))
    return out


@pytest.mark.parametrize("N", [2, 3, 4, 8])
@pytest.mark.parametrize("n", [1, 3, 7, 16, 17, 40, 64])
def test_restatement_equals_scalar_transcription(N, n):
    rng = np.random.default_rng(1000 * N + n)
    x = rng.standard_normal(n).astype(F32)
    want = scalar_spectra(x, N)
    Sr, Si = R.running_sums(x, N)
    vr, vi = R.demodulate_hann(Sr, Si, N)
    assert np.array_equal(vr.view(np.uint32), want[..., 0].view(np.uint32))
    assert np.array_equal(vi.view(np.uint32), want[..., 1].view(np.uint32))


@needs_ref
def test_full_restatement_uses_the_reference_phase_vocoder():
    x = np.random.default_rng(5).standard_normal((2, 50)).astype(F32)
    spv = R.analyze(x, 48000.0, 4)
    assert spv.shape == (2, 50, 4, 2)
    # frame 0 of bin b: phase_vocoder from a zero phase buffer -> f = b sr / N + ( phase - b / N pi2 ) sr / pi2 ... only finite here
    assert np.isfinite(spv).all()
    out = R.synthesize(spv, 48000.0)
    assert out.shape == (2, 50) and np.isfinite(out).all()


def test_twiddles_are_unit_and_match_the_definition():
    for N in (2, 3, 64, 1024):
        re, im = R.twiddles(N)
        ang = -2.0 * np.pi * np.arange(2 * N) / (2 * N)
        assert np.max(np.abs(re - np.cos(ang))) < 2e-6 * max(1, N / 256)
        assert np.max(np.abs(im - np.sin(ang))) < 2e-6 * max(1, N / 256)


def test_restatement_follows_the_identity_and_drifts_with_length():
    """F[f] = D_f (the trailing window's DFT) in exact arithmetic; the fp32 running sum drifts away from it as f grows."""
    N = 32
    L = 2 * N
    n = 400 * L
    x = np.random.default_rng(7).standard_normal(n).astype(F32)
    Sr, Si = R.running_sums(x, N)
    early = np.arange(L, 4 * L)
    late = np.arange(n - 3 * L, n)
    errs = []
    for fr in (early, late):
        vr, vi = R.demodulate_hann(Sr[fr], Si[fr], N, frames=fr)
        V = R.truth_spectra(x, N, fr)
        got = vr.astype(np.float64) + 1j * vi.astype(np.float64)
        errs.append(np.sqrt(np.sum(np.abs(got - V) ** 2) / np.sum(np.abs(V) ** 2)))
    print("restatement vs fp64 truth, N = %d: relative rms %.3e at frames [L, 4L), %.3e at the last 3L of %d" % (N, errs[0], errs[1], n))
    assert errs[0] < 1e-5
    assert errs[1] > errs[0]
