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


# ---------------------------------------------------------------------------------------------------------------------------------
# The numpy synthesis: inverse_phases / synthesize_np / synthesis_truth (no oracle/_ref needed)
# ---------------------------------------------------------------------------------------------------------------------------------

def _oracle_inverse(f, m, ar, phase0):
    """the project's own scalar inverse_phase_vocoder (oracle/flan_oracle.cpp), one call per MF: phases float64 and re float32, [n][K]"""
    import ctypes as C
    n, K = f.shape
    ph = np.empty((n, K), np.float64)
    re = np.empty((n, K), F32)
    r, i = C.c_float(), C.c_float()
    for b in range(K):
        buf = C.c_double(float(phase0[b]))
        for k in range(n):
            O.lib.oracle_inverse_phase_vocoder(C.byref(buf), float(m[k, b]), float(f[k, b]), float(ar), C.byref(r), C.byref(i))
            ph[k, b], re[k, b] = buf.value, r.value
    return ph, re


@pytest.mark.parametrize("ar", [8000.0, 44100.0, 48000.0, 192000.0])
def test_phase_recurrence_equals_the_oracle_to_the_bit(ar):
    """random (m, f, start phase): f of both signs from 1e-3 to 1e20 Hz and plain audio frequencies, start phases negative, inside
    [0, pi2], beyond it and huge.  The phase to the bit; the real part within one ulp of m (the restatement's cosine is the correctly
    rounded one, libm's cosf is within an ulp of it, and the product then rounds at most one ulp of m apart)."""
    rng = np.random.default_rng(int(ar))
    n, K = 12, 300
    f = (rng.choice([-1.0, 1.0], (n, K)) * 10.0 ** rng.uniform(-3.0, 20.0, (n, K))).astype(F32)
    f[:, :100] = rng.uniform(-ar, 2.0 * ar, (n, 100))
    f[0, 100], f[3, 101] = F32(1e20), F32(-1e20)
    m = (10.0 ** rng.uniform(-3.0, 0.0, (n, K))).astype(F32)
    phase0 = np.concatenate([rng.uniform(-50.0, 0.0, 60), rng.uniform(0.0, 6.3, 120), rng.uniform(6.3, 1e4, 60), 10.0 ** rng.uniform(5.0, 17.0, 60)])
    want_ph, want_re = _oracle_inverse(f, m, ar, phase0)
    got_ph = R.inverse_phases(f, ar, phase0)
    assert np.array_equal(got_ph.view(np.uint64), want_ph.view(np.uint64))
    got_re = (m * R.cos_f32(got_ph.astype(F32))).astype(F32)
    ulps = np.abs(got_re.astype(np.float64) - want_re) / np.spacing(m).astype(np.float64)
    print("inverse_phases vs the oracle at ar = %.0f: %d phases bit-identical, re within %.2f ulp of m (%d of %d differ)"
          % (ar, got_ph.size, ulps.max(), np.count_nonzero(ulps), ulps.size))
    assert ulps.max() <= 1.0


def test_the_fold_is_by_the_float_two_pi_and_never_of_a_negative_phase():
    P = float(R.PI2)
    ph = R.inverse_phases(np.array([[36000.0], [36000.0], [-100000.0], [1000.0]], F32), 48000.0)[:, 0]
    step = float(F32(F32(36000.0) / F32(48000.0)) * R.PI2)
    assert ph[0] == step and ph[1] == np.fmod(2 * step, P) and ph[1] != np.fmod(2 * step, 2.0 * np.pi)
    assert ph[2] < -6.0 and ph[3] < -6.0                              # below -pi2 and left there
    with np.errstate(invalid="ignore"):
        assert np.isnan(R.inverse_phases(np.array([[np.inf], [0.0]], F32), 48000.0)).all()      # fmod( inf ) is NaN, and stays
        assert np.isnan(R.inverse_phases(np.array([[np.nan], [0.0]], F32), 48000.0)).all()
    assert np.isneginf(R.inverse_phases(np.array([[-np.inf]], F32), 48000.0)).all()


def _sum_allowance(spv):
    """what two fp32 bin-order sums may differ by when each term differs by at most one ulp of its m: the terms' ulps, and for each of
    the N additions of either sum half an ulp of the largest partial sum possible, sum_b m"""
    m = spv[..., 0]
    N = m.shape[-1]
    total = np.sum(m.astype(np.float64), axis=-1)
    return 2.0 * (np.sum(np.spacing(m).astype(np.float64), axis=-1) + N * np.spacing(total.astype(F32)).astype(np.float64))


@needs_ref
def test_synthesize_np_equals_the_reference_translation_units():
    """3 channels x 60 frames x 9 bins, f of both signs, one 2.5e13 Hz and one 1e20 Hz MF: phases to the bit and terms within one ulp of m
    against the reference's own inverse_phase_vocoder, the sum against R.synthesize within the allowance that follows"""
    rng = np.random.default_rng(77)
    ch, n, N = 3, 60, 9
    spv = np.empty((ch, n, N, 2), F32)
    spv[..., 0] = 10.0 ** rng.uniform(-3.0, 0.0, (ch, n, N))
    spv[..., 1] = rng.uniform(-24000.0, 96000.0, (ch, n, N))
    spv[1, 20, 4, 1], spv[2, 31, 0, 1] = R.HUGE_F
    ref = O.load_ref()
    ph = R.inverse_phases(spv[..., 1], 48000.0)
    for c in range(ch):
        buf = np.zeros(N, np.float64)
        for k in range(n):
            rr, ii = np.empty(N, F32), np.empty(N, F32)
            m = np.ascontiguousarray(spv[c, k, :, 0])
            ref.ref_inverse_phase_vocoder_batch(N, buf, m, np.ascontiguousarray(spv[c, k, :, 1]), F32(48000.0), rr, ii)
            assert np.array_equal(buf.view(np.uint64), ph[c, k].view(np.uint64)), (c, k)
            mine = (m * R.cos_f32(ph[c, k].astype(F32))).astype(F32)
            assert np.all(np.abs(mine.astype(np.float64) - rr) <= np.spacing(m)), (c, k)
    got, want = R.synthesize_np(spv, 48000.0), R.synthesize(spv, 48000.0)
    d = np.abs(got.astype(np.float64) - want)
    print("synthesize_np vs the reference's synthesis: max |d| %.3e (allowance at that sample %.3e)" % (d.max(), _sum_allowance(spv).flat[np.argmax(d)]))
    assert np.all(d <= _sum_allowance(spv))


@needs_ref
def test_analyze_frames_equals_the_rows_of_analyze():
    x = np.random.default_rng(6).standard_normal(70).astype(F32)
    frames = [1, 2, 9, 10, 11, 40, 69]
    whole = R.analyze(x[None, :], 48000.0, 5)[0]
    assert np.array_equal(R.analyze_frames(x, 48000.0, 5, frames).view(np.uint32), whole[frames].view(np.uint32))


def _pipeline_stand_ins():
    """what the GPU tests take from the device analysis, here from the fp64 truth of the same noise: as is, repitched, set"""
    for N in (100, 513):
        n = 8 * N + 37
        x = (0.5 * np.random.default_rng(N).standard_normal((2, n))).astype(F32)
        spv = R.truth_spv(x, N, 48000.0)
        for tag, f in (("as is", spv[..., 1]), ("x 1.25", spv[..., 1] * F32(1.25)), ("x 0.8", spv[..., 1] * F32(0.8)), ("= 440.5", np.full_like(spv[..., 1], 440.5))):
            out = spv.copy()
            out[..., 1] = f
            yield "pipeline N=%d %s" % (N, tag), N, out


def test_the_restatements_own_error_on_every_synthesis_case():
    """synthesize_np against synthesis_truth on the whole table of tests/test_gpu_spv_synthesis.py: what the fp32 cosine, product and
    bin-order sum cost.  The bound is reasoning, not measurement: two roundings a term, and the N partial-sum roundings of 2^-24 of a
    partial sum that walks at random to sqrt( N ) terms' size add up to about sqrt( N ) / 2.4 of them relative to the sum; 2 + sqrt( N )."""
    rows = [(c["name"], c["N"]) + R.synthesis_errors(*R.syn_expected(c["name"])) for c in R.SYN_CASES]
    for name, N, spv in _pipeline_stand_ins():
        ph = R.inverse_phases(spv[..., 1], 48000.0)
        rows.append((name, N) + R.synthesis_errors(R.synthesize_np(spv, 48000.0, ph), R.synthesis_truth(spv, 48000.0, ph)))
    for name, N, rms, mx in rows:
        print("own error %-24s N=%-5d rel rms %.3e  max/peak %.3e" % (name, N, rms, mx))
        assert 0.0 < rms <= 2.0 ** -24 * (2.0 + np.sqrt(N)) and np.isfinite(mx), name


def test_the_case_table_reaches_every_synthesis_variant():
    """K = ceil( N / 256 ) -> k_spv_synthesize<1, 2, 4, 8, 16, 0>; both sincos branches and both folds in the extreme cases"""
    ks = {min(k for k in (1, 2, 4, 8, 16, 99) if -(-c["N"] // 256) <= k) for c in R.SYN_CASES}
    assert ks == {1, 2, 4, 8, 16, 99}
    ph = R.inverse_phases(R.spv_case("sincos_wide")[..., 1], 48000.0).astype(F32)
    assert (np.abs(ph) >= 2.0 ** 22).any() and (np.abs(ph) < 2.0 ** 22).any()
    f = R.spv_case("fold_any")[..., 1]
    assert np.count_nonzero(f == F32(2.5e13)) == 10 and np.count_nonzero(f == F32(1e20)) == 10
    assert F32(2.5e13) / F32(48000.0) * R.PI2 > 3e9
    assert R.inverse_phases(R.spv_case("negative")[..., 1], 48000.0).min() < -50.0
