"""Audio::synthesize_spectrum on the MI355X (flan_amd/csrc/spectrum.hip, the generalised loop of wavetable.hip): the table against the fp64
truth, the loop against the vectors the reference's own WDL_Resampler made (tests/golden/ref_made/wdl_spectrum.npz), against the Python
restatement (tests/spectrum_reference.py) and against flanhip_wavetable_synth over the rotated table, the whole call against the restatement
applied to the device's own table.  DESIGN.md 4.24 lists the measured values.

Table: the relative-max error (max |error| / max |truth|) is at most 4 x the single-precision stand-in's on the same spectrum, with a floor
of 4 fp32 ulp (2^-22): the bound test_gpu_wavetable.py holds its transform to.
Measured on the device (error / bound; the device's relative-max error against the stand-in's):
  p = 6: 0.58 (2.0e-7 against 0.9e-7)    p = 13: 0.26 (1.9e-7 against 1.8e-7)    p = 14: 0.26 (1.9e-7 against 1.8e-7)
  p = 15: 0.26 (2.0e-7 against 1.9e-7)   p = 20: 0.29 (2.0e-7 against 1.8e-7)    p = 22: 0.29 (2.6e-7 against 2.3e-7)
One bin against its closed form: at most 3.7e-7 of the amplitude (p = 17, bin 4097).
Synthesis: bit-identical to the reference-made outputs, to the restatement and to flanhip_wavetable_synth (bound 0)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import spectrum_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
TABLE_FACTOR, TABLE_FLOOR = 4.0, 2.0 ** -22
# p = 6: the smallest; 13: the largest of one workgroup; 14: the smallest of two passes (C1 x C2 = 16 x 512); 15: 16 x 1024; 20: the default
# (128 x 4096; the split is C1 = max( 16, C / 4096 )); 22: the largest C1 (512 x 4096).  The degenerate spectra add 17 (16 x 4096)
TABLE_POWERS = [6, 13, 14, 15, 20, 22]
FUNDAMENTAL_POWER = {6: 4, 13: 8, 14: 8, 15: 8, 20: 8, 22: 8}
CASES = R.load_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


_table_cache = {}


def table_case(p):
    """the default Gaussian spectrum of a size with seeded phases, its truth and stand-in, and the device's table (computed once)"""
    if p not in _table_cache:
        fp = FUNDAMENTAL_POWER[p]
        harmonic, _ = R.bins(p, fp)
        mag = R.magnitudes(p, fp)
        theta = R.phases(1000 + p, harmonic)
        _table_cache[p] = dict(mag=mag, theta=theta, harmonic=harmonic, truth=R.table_truth(mag, theta), standin=R.table_standin(mag, theta),
                               table=fa.spectrum_table(mag, theta, p))
    return _table_cache[p]


@pytest.mark.parametrize("p", TABLE_POWERS)
def test_table_against_the_truth(p):
    k = table_case(p)
    table, truth = k["table"], k["truth"]
    assert table.shape == truth.shape and not np.any(np.isnan(table))
    scale = np.max(np.abs(truth))
    err = np.max(np.abs(table.astype(np.float64) - truth)) / scale
    own = np.max(np.abs(k["standin"].astype(np.float64) - truth)) / scale
    bound = max(TABLE_FACTOR * own, TABLE_FLOOR)
    print("p=%d: rel max %.3e (stand-in %.3e, bound %.3e), error / bound = %.3f" % (p, err, own, bound, err / bound))
    assert err <= bound, (p, err, own)


def one_bin(p, k, r=0.75, theta=0.0):
    B = R.sizes(p)[2]
    mag, th = np.zeros(B, F32), np.zeros(B, F32)
    mag[k], th[k] = r, theta
    return mag, th


@pytest.mark.parametrize("p", [6, 13, 14, 17])
def test_degenerate_spectra(p):
    N, C, B = R.sizes(p)
    n = np.arange(N)
    # one bin: 2 r cos( 2 pi k n / N + theta ) with the fp32 theta.  Bound 2^-20 of the amplitude: 16 roundings of 2^-24 -- the fp32 X, the
    # pre-merge's twiddle and sums, the inter-pass twiddle and up to six butterfly stages each rounding once or twice -- added as if all aligned
    for k, theta in ((1, 0.0), (C // 2, 1.25), (C - 1, 4.0), (min(C - 3, 4097), 2.0)):
        mag, th = one_bin(p, k, 0.75, theta)
        got = fa.spectrum_table(mag, th, p).astype(np.float64)
        want = 2.0 * 0.75 * np.cos(2.0 * np.pi * ((k * n) % N) / N + float(F32(theta)))
        err = np.max(np.abs(got - want)) / 1.5
        print("p=%d bin %d: rel max %.3e" % (p, k, err))
        assert err <= 2.0 ** -20, (p, k, err)
    # bin 0: a constant; bin C: an alternating sign; both exact ( theta = 0: X = r )
    mag, th = one_bin(p, 0, 0.75)
    assert np.array_equal(fa.spectrum_table(mag, th, p), np.full(N, 0.75, F32))
    mag, th = one_bin(p, C, 0.75)
    assert np.array_equal(fa.spectrum_table(mag, th, p), np.where(n % 2 == 0, 0.75, -0.75).astype(F32))


@pytest.mark.parametrize("p", [6, 13, 14])
def test_imaginary_parts_of_bin_0_and_bin_c_change_nothing(p):
    k = table_case(p)
    mag, theta = k["mag"].copy(), k["theta"].copy()
    mag[0], mag[-1] = 0.5, 0.25                       # ( the Gaussian case has harmonic 0 at bin 0 )
    theta[0], theta[-1] = 0.0, 0.0
    base = fa.spectrum_table(mag, theta, p)
    # theta = 2^-13: cos rounds to 1 in fp32, so the real parts are the same numbers, beside imaginary parts of r 2^-13
    theta[0], theta[-1] = F32(2.0 ** -13), F32(2.0 ** -13)
    assert np.array_equal(bits(fa.spectrum_table(mag, theta, p)), bits(base))
    # and they do matter in every other bin: the same turn of the loudest one
    theta[1 + int(np.argmax(mag[1:-1]))] += F32(2.0 ** -13)
    assert not np.array_equal(bits(fa.spectrum_table(mag, theta, p)), bits(base))


def run_synth(c):
    return fa.spectrum_synth(c["table"], c["fundamental"], c["ch"], c["out_frames"], c["g"], c["freq"])


_synth_cache = {}


def synth_case(i):
    if i not in _synth_cache:
        _synth_cache[i] = run_synth(CASES[i])
    return _synth_cache[i]


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_synth_against_the_reference_made_output(i):
    c, y = CASES[i], synth_case(i)
    assert y.shape == c["out"].shape and not np.any(np.isnan(y))
    differ = int(np.sum(bits(y) != bits(c["out"])))
    print("%s: %d of %d samples differ" % (c["name"], differ, y.size))
    assert differ == 0
    plan = fa.spectrum_synth_plan(c["out_frames"], c["fundamental"], c["g"], c["freq"])
    assert np.array_equal(plan["wanted"], c["wanted"]) and np.array_equal(plan["num_out"], c["delivered"])


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_synth_against_the_restatement_and_the_wavetable_entry_point(i):
    c, y = CASES[i], synth_case(i)
    want = R.synth(c["table"], c["fundamental"], c["ch"], c["out_frames"], c["g"], c["freq"])
    assert np.array_equal(bits(y), bits(want))
    N = 1 << c["p"]
    sr = float(F32(c["fundamental"]) * F32(N))
    plan = fa.wavetable_synth_plan(c["out_frames"], sr, N, c["g"], c["freq"])
    index = np.zeros((1, plan["first_out"].size), F32)
    for ch in range(c["ch"]):
        assert fa.spectrum_jump(ch, c["ch"], c["p"]) == R.jump(ch, c["ch"], c["p"])
        row = fa.wavetable_synth(np.roll(c["table"], -R.jump(ch, c["ch"], c["p"]))[None], N, sr, c["out_frames"], c["g"], c["freq"], index, smooth=False)
        assert np.array_equal(bits(row[0]), bits(y[ch])), ch


def test_synth_on_a_device_made_table_of_the_default_size():
    """p = 20: the phase offsets and the wrap of a table the two-pass transform made"""
    p, fundamental, ch, frames, g = 20, 256.0, 3, 12000, 48
    freq = np.full(1, 7680.0, F32)                    # ratio 30: 360 000 input samples, which the third channel (from 699 050 on) reads across the period's end
    table = table_case(p)["table"]
    got = fa.spectrum_synth(table, fundamental, ch, frames, g, freq)
    want = R.synth(table, fundamental, ch, frames, g, freq)
    assert np.array_equal(bits(got), bits(want))


WHOLE = [(13, 8, 2, 4800, 48, 220.0), (14, 8, 3, 2400, 48, 1000.0), (16, 4, 1, 1000, 480, 30.0)]


@pytest.mark.parametrize("p,fp,ch,frames,g,f", WHOLE)
def test_whole_call(p, fp, ch, frames, g, f):
    harmonic, _ = R.bins(p, fp)
    mag, theta = R.magnitudes(p, fp), R.phases(77, harmonic)
    freq = np.full(1, f, F32)
    got = fa.audio_synthesize_spectrum(mag, theta, p, fp, ch, frames, g, freq)
    table = fa.spectrum_table(mag, theta, p)
    want, end = R.set_volume(R.synth(table, 2.0 ** fp, ch, frames, g, freq))
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want))
    assert end == frames - 1 and np.max(np.abs(got[:, :end])) == 1.0


def test_host_and_device_forms_are_bit_identical_and_repeat():
    dev = torch.device("cuda", 0)
    for p in (13, 15):
        k = table_case(p)
        B, N = k["mag"].size, 1 << p
        d_mag, d_theta = torch.from_numpy(k["mag"]).to(dev), torch.from_numpy(k["theta"]).to(dev)
        d_table = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
        d_ws = torch.full((fa.spectrum_table_workspace_bytes(p),), 0xFF, dtype=torch.uint8, device=dev)
        fa.spectrum_table_dev(d_mag, d_theta, p, d_table, d_ws)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_table.cpu().numpy()), bits(k["table"])), p
        assert np.array_equal(bits(fa.spectrum_table(k["mag"], k["theta"], p)), bits(k["table"])), p
        fp, ch, frames, g, freq = 8, 3, 2400, 48, np.full(1, 330.0, F32)
        host = fa.spectrum_synth(k["table"], 256.0, ch, frames, g, freq)
        d_out = torch.full((ch, frames), float("nan"), dtype=torch.float32, device=dev)
        d_ws2 = torch.full((fa.spectrum_synth_workspace_bytes(p, 256.0, ch, frames, g, freq),), 0xFF, dtype=torch.uint8, device=dev)
        fa.spectrum_synth_dev(d_table, p, 256.0, ch, frames, g, freq, d_out, d_ws2)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(host)), p
        assert np.array_equal(bits(fa.spectrum_synth(k["table"], 256.0, ch, frames, g, freq)), bits(host)), p
        whole = fa.audio_synthesize_spectrum(k["mag"], k["theta"], p, fp, ch, frames, g, freq)
        d_out.fill_(float("nan"))
        d_ws3 = torch.full((fa.audio_synthesize_spectrum_workspace_bytes(p, fp, ch, frames, g, freq),), 0xFF, dtype=torch.uint8, device=dev)
        fa.audio_synthesize_spectrum_dev(d_mag, d_theta, p, fp, ch, frames, g, freq, d_out, d_ws3)
        torch.cuda.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(whole)), p
        assert np.array_equal(bits(fa.audio_synthesize_spectrum(k["mag"], k["theta"], p, fp, ch, frames, g, freq)), bits(whole)), p
