"""flan_amd/csrc/volume.hip and the C++ methods over it on the MI355X against tests/volume_reference.py.

Exact paths (ring_modulate, the fades, invert_phase, square / saw / triangle, the ADSR envelopes, white noise, every composition) are compared bit
for bit.  The numeric paths are held to the fp64 truth with derived bounds:
  phases      circular distance to the sequential fp64 modular sum <= 2^-23 of a cycle: the fp64 scan's own error over <= 10^7 terms is below
              10^-9 of a cycle, the division and the one rounding to fp32 cost at most 2^-24 each on [0, 1)
  sine, the moisture shaper      with a the truth and b the fp32 restatement of the same case, E_ref = max |b - a|: max |device - a| <= 2 E_ref
              (both round the same fp32 product chain, which dominates; the ratio is printed)
  energy      within one fp32 ulp of the exactly summed squares
  envelope    the bounds tests/test_gpu_convolve.py holds the convolution to against its own truth
Outputs and workspaces are pre-filled with 0xFF bytes or a sentinel and nothing may be written past an output."""
import os
import tempfile

import numpy as np
import pytest
import torch  # noqa: F401  (first: the library then binds to the HIP runtime torch loaded, as in the rest of the suite)

import flan_amd as fa
import convolve_reference as R
import host_cpp
import oracle_lib as O
import volume_reference as V

pytestmark = pytest.mark.gpu
F32 = np.float32
SR = 48000.0
GUARD = 8                                   # floats behind every output that must keep their sentinel
SENTINEL = F32(-7.25)
HB_CHAIN_BOUND = 1.2e-7                     # tests/test_gpu_resample.py::test_resample_half_band_chains: max |device - restatement|


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def uniform(shape, seed, lo=-1.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, shape).astype(F32)


class Out:
    """a device output of `count` floats, `offset` floats into its block, with GUARD sentinels on both sides"""

    def __init__(self, count, offset=0):
        self.count, self.offset = count, GUARD + offset
        self.total = self.offset + count + GUARD
        self.block = fa.DeviceArray(host=np.full(self.total, SENTINEL, F32))
        self.ptr = self.block.ptr + 4 * self.offset

    def host(self, shape=None):
        whole = self.block.to_host(self.total)
        assert np.all(whole[:self.offset] == SENTINEL) and np.all(whole[self.offset + self.count:] == SENTINEL), "written outside the output"
        got = whole[self.offset:self.offset + self.count]
        return got if shape is None else got.reshape(shape)


def placed(x, offset=0):
    """x on the device, `offset` floats into its block: ( block, pointer )"""
    flat = np.concatenate([np.zeros(offset, F32), np.ascontiguousarray(x, F32).reshape(-1)])
    block = fa.DeviceArray(host=flat)
    return block, block.ptr + 4 * offset


# ---- ring_modulate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,other,offset", [((3, 1001), (2, 37), 0), ((3, 1001), (2, 37), 1), ((2, 100), (1, 250), 3), ((1, 1), (1, 1), 0), ((1, 3), (4, 2), 2), ((2, 5000), (3, 4099), 0)])
def test_ring_modulate(shape, other, offset):
    x, m = uniform(shape, 1), uniform(other, 2)
    keep_x, px = placed(x, offset)
    d_m = fa.DeviceArray(host=m)
    out = Out(x.size, offset)
    fa.audio_ring_modulate_dev(px, shape[0], shape[1], d_m, other[0], other[1], out.ptr)
    assert np.array_equal(bits(out.host(shape)), bits(V.ring_modulate(x, m)))
    fa.audio_ring_modulate_dev(px, shape[0], shape[1], d_m, other[0], other[1], px)        # in place
    assert np.array_equal(bits(keep_x.to_host(offset + x.size)[offset:]), bits(V.ring_modulate(x, m).reshape(-1)))


# ---- invert_phase: flanhip_audio_gain_dev with -1 ----------------------------------------------------------------------------------------------
def test_invert_phase_is_the_sign_bit():
    x = uniform((2, 1003), 3)
    x[0, :6] = [0.0, -0.0, 1e-41, -1e-41, np.inf, -np.inf]
    x[1, 1002] = np.inf
    d_x = fa.DeviceArray(host=x)
    out = Out(x.size)
    fa.audio_gain_dev(d_x, 2, 1003, -1.0, out.ptr)
    assert np.array_equal(bits(out.host((2, 1003))), bits(x) ^ np.uint32(0x80000000))


# ---- the fades ----------------------------------------------------------------------------------------------------------------------------
INTERPS = {"sqrt": V.interp_sqrt, "linear": V.interp_linear, "callable": lambda v: F32(F32(v) * F32(v))}
FADE_CASES = [(16, 16), (0, 7), (7, 0), (0, 0), (700, 700), (-3, -4)]


def fade_on_device(x, start, end, interp, offset=0, in_place=False):
    ch, n = x.shape
    start, end = fa.fade_frames_plan(n, start, end)
    assert (start, end) == V.fade_plan(n, start, end)
    s, e = V.fade_tables(start, end, interp)
    d_s = fa.DeviceArray(host=s) if start else None
    d_e = fa.DeviceArray(host=e) if end else None
    keep, px = placed(x, offset)
    if in_place:
        fa.audio_fade_dev(px, ch, n, d_s, start, d_e, end, px)
        return keep.to_host(offset + x.size)[offset:].reshape(ch, n)
    out = Out(x.size, offset)
    fa.audio_fade_dev(px, ch, n, d_s, start, d_e, end, out.ptr)
    return out.host((ch, n))


@pytest.mark.parametrize("name", sorted(INTERPS))
def test_fade_kernel(name):
    x = uniform((2, 1000), 4)
    for start, end in FADE_CASES:
        want = V.fade_frames(x, start, end, INTERPS[name])
        assert np.array_equal(bits(fade_on_device(x, start, end, INTERPS[name])), bits(want)), (start, end)
    assert np.array_equal(V.fade_frames(x, 0, 0, INTERPS[name]), x) and V.fade_plan(1000, 700, 700) == (500, 500)
    # rows at an odd float offset, a ragged length, the output in place, fades that overlap fully ( 3 x 333 with 333 + 333 > 333 )
    y = uniform((3, 333), 5)
    for offset in (1, 2, 3):
        assert np.array_equal(bits(fade_on_device(y, 50, 21, INTERPS[name], offset)), bits(V.fade_frames(y, 50, 21, INTERPS[name])))
    assert np.array_equal(bits(fade_on_device(y, 50, 21, INTERPS[name], 1, in_place=True)), bits(V.fade_frames(y, 50, 21, INTERPS[name])))
    # both ranges cover a frame: the start's gain first, then the end's (the C ABI takes what the shrink never produces)
    s, e = V.fade_tables(6, 5, INTERPS[name])
    z = uniform((2, 7), 6)
    want = z.copy()
    want[:, :6] = want[:, :6] * s
    want[:, 2:] = want[:, 2:] * e[::-1]
    out = Out(z.size)
    fa.audio_fade_dev(fa.DeviceArray(host=z), 2, 7, fa.DeviceArray(host=s), 6, fa.DeviceArray(host=e), 5, out.ptr)
    assert np.array_equal(bits(out.host((2, 7))), bits(want))
    one = uniform((1, 1), 7)
    assert np.array_equal(bits(fade_on_device(one, 1, 0, INTERPS[name])), bits(V.fade_frames(one, 1, 0, INTERPS[name])))


# ---- the C++ methods' results, written by tests/cpp/volume_test.cpp --dump --------------------------------------------------------------------
POOL = uniform(40200, 11)


def take(ch, n):
    return POOL[:ch * n].reshape(ch, n).copy()


@pytest.fixture(scope="module")
def dumped():
    host_cpp.build("volume_test")
    with tempfile.TemporaryDirectory() as d:
        POOL.tofile(os.path.join(d, "in.raw"))
        host_cpp.run("volume_test", "--dump", os.path.join(d, "in.raw"), d)
        out = {}
        for f in os.listdir(d):
            if f.endswith(".bin"):
                raw = open(os.path.join(d, f), "rb").read()
                ch, n = np.frombuffer(raw[:8], np.int32)
                out[f[:-4]] = (np.frombuffer(raw[12:], F32).reshape(ch, n).copy(), float(np.frombuffer(raw[8:12], F32)[0]))
    return out


def test_cpp_fades(dumped):
    x = take(2, 1000)
    for name, interp in INTERPS.items():
        for start, end in FADE_CASES:
            got, sr = dumped["fade_%s_%d_%d" % (name, start, end)]
            assert sr == SR and np.array_equal(bits(got), bits(V.fade_frames(x, start, end, interp))), (name, start, end)
    assert np.array_equal(bits(dumped["fade_sqrt_0_0"][0]), bits(x)) and np.array_equal(bits(dumped["fade_linear_-3_-4"][0]), bits(x))
    assert np.array_equal(bits(dumped["fade_rows_333"][0]), bits(V.fade_frames(take(3, 333), 50, 21, V.interp_sqrt)))
    # fade( seconds ) is fade_frames( time_to_frame ): Frame( 0.004f * 48000.0f ), Frame( 0.0015f * 48000.0f )
    s, e = int(F32(0.004) * F32(SR)), int(F32(0.0015) * F32(SR))
    assert np.array_equal(bits(dumped["fade_seconds"][0]), bits(V.fade_frames(x, s, e, V.interp_linear)))


def test_cpp_ring_and_invert(dumped):
    assert np.array_equal(bits(dumped["ring"][0]), bits(V.ring_modulate(take(3, 1001), take(2, 37))))
    assert np.array_equal(bits(dumped["invert"][0]), bits(take(2, 1000)) ^ np.uint32(0x80000000))


def test_cpp_adsr(dumped):
    """apply_adsr_envelope is modify_volume of the restated envelope sampled in fp32 at f * ( 1.0f / sr ).  At a sample rate of 16 every time is
    exact: frames 8, 12, 28 and 32 sit on the segment boundaries and frames 33 ... 63 are past a + d + s + r"""
    x = take(2, 64)
    t = [F32(f) * (F32(1.0) / F32(16.0)) for f in range(64)]
    assert float(t[8]) == 0.5 and float(t[12]) == 0.75 and float(t[28]) == 1.75 and float(t[32]) == 2.0
    gain = np.array([V.adsr(v, 0.5, 0.25, 1.0, 0.25, 0.5) for v in t], F32)        # exponents of 1: pow( x, 1 ) is x in every library
    assert gain[8] == 1 and gain[12] == 0.5 and gain[28] == 0.5 and gain[32] == 0 and np.all(gain[33:] == 0) and gain[4] == 0.5 and gain[30] == 0.25
    got, sr = dumped["adsr"]
    assert sr == 16.0 and np.array_equal(bits(got), bits(x * gain))
    gain = np.array([V.adsr(v, 0.5, 0, 0, 1.5, 1) for v in t], F32)
    assert gain[8] == 1 and gain[20] == 0.5 and gain[32] == 0
    assert np.array_equal(bits(dumped["ar"][0]), bits(x * gain))
    y = take(2, 1000)
    t = [F32(f) * (F32(1.0) / F32(SR)) for f in range(1000)]
    gain = np.array([V.adsr(v, 0.004, 0.003, 0.005, 0.006, 0.3, 1.5, 2.0, 0.7) for v in t], F32)
    got = dumped["adsr_48k"][0]
    # powf with fractional exponents: the C library's and numpy's are each within an ulp of the power, a value of at most 1: 2 x 2^-24 apart,
    # times a sample of at most 1, and each product rounds once more, 2^-25 each
    assert np.max(np.abs(got - y * gain)) <= 2.0 ** -23 + 2.0 ** -24


# ---- the named waveforms at given phases ------------------------------------------------------------------------------------------------------
def phases_for_waveforms():
    rng = np.random.default_rng(21)
    return np.concatenate([rng.uniform(0, 1, 20001), rng.uniform(-700, 700, 5000), [0.0, 0.25, 0.5, 0.75, 1.0, -0.25, -0.5, -1.0, 603.18578]]).astype(F32)


def waveform_on_device(kind, t, offset=0):
    keep, pt = placed(t, offset)
    out = Out(t.size, offset)
    fa.waveform_dev(kind, pt, t.size, out.ptr)
    return out.host()


@pytest.mark.parametrize("kind", [V.SQUARE, V.SAW, V.TRIANGLE])
def test_square_saw_triangle_are_the_restatement(kind):
    t = phases_for_waveforms()
    for offset in (0, 1):
        assert np.array_equal(bits(waveform_on_device(kind, t, offset)), bits(V.waveform(kind, t)))


def test_sine_at_given_phases():
    t = phases_for_waveforms()
    a, b = V.waveform_truth(V.SINE, t), V.waveform(V.SINE, t)
    e_ref = np.max(np.abs(b - a))
    dev = np.max(np.abs(waveform_on_device(V.SINE, t) - a))
    print("\nsine: E_ref %.3e  device %.3e  ratio %.3f" % (e_ref, dev, dev / e_ref))
    assert dev <= 2 * e_ref


# ---- the oscillator's phases --------------------------------------------------------------------------------------------------------------
M = 768000.0


def frequencies(kind, n):
    if kind == "constant":
        return 440.0
    if kind == "negative":
        return -1234.5
    if kind == "sweep":
        return np.linspace(20.0, 20000.0, n).astype(F32)
    return (3000.0 * np.sin(np.arange(n) * (2 * np.pi / 1500.0)) + 100.0).astype(F32)              # crosses 0 again and again


def phases_on_device(freq, n, run=0, wave_kind=None):
    with fa.osc_run_forced(run):
        d_ws = fa.DeviceArray(host=np.full(fa.osc_workspace_bytes(n), 0xFF, np.uint8))
        d_f = freq if np.isscalar(freq) else fa.DeviceArray(host=freq)
        ph, wv = Out(n), Out(n) if wave_kind is not None else None
        fa.osc_phase_dev(d_f, n, M, ph.ptr, None if wv is None else wv.ptr, -1 if wave_kind is None else wave_kind, d_ws)
        return ph.host(), None if wv is None else wv.host()


PHASE_TRUTH = {}


def phase_truth(kind, n):
    if (kind, n) not in PHASE_TRUTH:
        f = frequencies(kind, n)
        PHASE_TRUTH[kind, n] = V.phases_truth(np.full(n, f, F32) if np.isscalar(f) else f, M)
    return PHASE_TRUTH[kind, n]


@pytest.mark.parametrize("kind", ["constant", "sweep", "negative", "crossing"])
@pytest.mark.parametrize("n,run", [(4095, 0), (4096, 0), (4097, 0), (65536 + 257, 1), (4097, 3), (1, 0)])
def test_phases_against_the_fp64_truth(kind, n, run):
    if run == 0:
        assert fa.osc_block_frames() == 4096                        # 4095 / 4096 / 4097: one block, its last frame, one frame into the next
    else:
        assert 65536 + 257 > fa.osc_carry_pass_blocks() * 256      # run 1: past the first 256-block pass of k_scan_carry
    got, _ = phases_on_device(frequencies(kind, n), n, run)
    d = V.circular_distance(got, phase_truth(kind, n)).max()
    print("\nphases %s n=%d run=%d: %.3e of a cycle (bound %.3e)" % (kind, n, run, d, 2.0 ** -23))
    assert d <= 2.0 ** -23
    assert got.min() >= 0 and got.max() <= 1 and got[0] == 0


def test_the_fused_waveform_is_the_waveform_at_the_phases():
    n = 4097
    for kind in (V.SINE, V.SQUARE, V.SAW, V.TRIANGLE):
        ph, wv = phases_on_device(frequencies("sweep", n), n, 0, kind)
        assert np.array_equal(bits(wv), bits(waveform_on_device(kind, ph)))
        only_wave = Out(n)
        d_ws = fa.DeviceArray(host=np.full(fa.osc_workspace_bytes(n), 0xFF, np.uint8))
        fa.osc_phase_dev(fa.DeviceArray(host=frequencies("sweep", n)), n, M, None, only_wave.ptr, kind, d_ws)
        assert np.array_equal(bits(only_wave.host()), bits(wv))


def test_oscillator_chain_with_an_explicit_length():
    """the decimation is the restated chain applied to the device's own wave samples, at the length the caller names; the whole call adds nothing"""
    length, over = 0.05, 16
    n, n_in, in_rate = fa.synthesize_waveform_frames(length, SR, over)
    assert (n, n_in, in_rate) == (2400, 38400, M)
    d_ws = fa.DeviceArray(host=np.full(fa.osc_workspace_bytes(n_in), 0xFF, np.uint8))
    wave = Out(n_in)
    fa.osc_phase_dev(440.0, n_in, in_rate, None, wave.ptr, V.SAW, d_ws)
    w = wave.host()
    out = Out(n)
    fa.oneshot_resample_dev(wave.ptr, n_in, in_rate, SR, out.ptr, n)
    staged = out.host()
    ref = O.resample_chain(w[None, :], in_rate, SR)
    assert ref.shape == (1, n)
    assert np.max(np.abs(staged.astype(np.float64) - ref[0])) <= HB_CHAIN_BOUND
    whole = Out(n)
    d_ws2 = fa.DeviceArray(host=np.full(fa.audio_synthesize_waveform_workspace_bytes(length, SR, over), 0xFF, np.uint8))
    fa.audio_synthesize_waveform_dev(V.SAW, 440.0, length, SR, over, whole.ptr, d_ws2)
    assert np.array_equal(bits(whole.host()), bits(staged))
    # a shorter length than Audio::resample would choose: the same samples, fewer of them
    short = Out(n - 100)
    fa.oneshot_resample_dev(wave.ptr, n_in, in_rate, SR, short.ptr, n - 100)
    assert np.array_equal(bits(short.host()), bits(staged[:n - 100]))
    # equal rates: the samples pass through, zeros behind the input's end
    same = Out(50)
    fa.oneshot_resample_dev(wave.ptr, 40, SR, SR, same.ptr, 50)
    got = same.host()
    assert np.array_equal(bits(got[:40]), bits(w[:40])) and np.all(got[40:] == 0)


def test_cpp_oscillator_and_noise(dumped):
    got, sr = dumped["osc_saw"]
    n, n_in, in_rate = fa.synthesize_waveform_frames(0.05, SR, 16)
    whole = Out(n)
    d_ws = fa.DeviceArray(host=np.full(fa.audio_synthesize_waveform_workspace_bytes(0.05, SR, 16), 0xFF, np.uint8))
    fa.audio_synthesize_waveform_dev(V.SAW, 440.0, 0.05, SR, 16, whole.ptr, d_ws)
    assert sr == SR and got.shape == (1, n) and np.array_equal(bits(got[0]), bits(whole.host()))
    noise, sr = dumped["noise_77"]
    drawn = V.white_noise_draw(77, int(F32(0.02) * F32(SR * 4)))
    assert np.array_equal(bits(fa.white_noise_draw(77, drawn.size)), bits(drawn))
    assert sr == SR and np.array_equal(bits(noise), bits(fa.resample(drawn[None, :], SR * 4, SR)))


# ---- the moisture shaper --------------------------------------------------------------------------------------------------------------------
def moisture_on_device(s, n, amount, frequency, skew, kind=V.SINE, sr_over=4 * SR, sr=SR, spare=0):
    """s: [ch][n_over]; curves: floats or arrays of n floats (uploaded with `spare` poisoned floats behind them)"""
    ch, n_over = s.shape
    keep = []

    def arg(v):
        if np.isscalar(v):
            return float(v)
        keep.append(fa.DeviceArray(host=np.concatenate([np.asarray(v, F32), np.full(spare, 1e30, F32)])))
        return keep[-1]
    out = Out(s.size)
    fa.audio_moisture_dev(fa.DeviceArray(host=s), ch, n_over, sr_over, n, sr, arg(amount), arg(frequency), arg(skew), kind, out.ptr)
    return out.host((ch, n_over))


def moisture_case(frequency, curves):
    n_over = 100001
    n = (n_over + 3) // 4
    s = uniform((2, n_over), 31)
    s[0, :6] = [0.0, 1.0, -1.0, -0.5, 0.5, -0.0]
    s[1, -3:] = [1.0, -1.0, 0.0]
    if curves:
        t = np.arange(n) / n
        amount, frequency, skew = (0.2 + 0.6 * t).astype(F32), (frequency * (0.25 + 0.75 * t)).astype(F32), (1.5 + 3.0 * t).astype(F32)
    else:
        amount, skew = 0.5, 4.0
    F = np.broadcast_to(np.arange(n_over), s.shape)
    args = (s, F, 4 * SR, SR, n, amount, frequency, skew)
    return s, n, (amount, frequency, skew), V.moisture_truth(*args), V.moisture(*args)


@pytest.mark.parametrize("frequency,curves", [(96.0, False), (3.0, False), (96.0, True), (3.0, True)])
def test_moisture_kernel_against_the_truth(frequency, curves):
    s, n, (amount, freq, skew), a, b = moisture_case(frequency, curves)
    e_ref = np.max(np.abs(b - a))
    got = moisture_on_device(s, n, amount, freq, skew, spare=4)
    dev = np.max(np.abs(got - a))
    print("\nmoisture frequency %g %s: E_ref %.3e  device %.3e  ratio %.3f  bit-identical to the restatement %.4f"
          % (frequency, "curves" if curves else "constants", e_ref, dev, dev / e_ref, np.mean(bits(got) == bits(b))))
    assert dev <= 2 * e_ref
    assert got[0, 0] == 0 and np.signbit(got[0, 5]) and got[1, -1] == 0                  # s = 0 and -0 stay


@pytest.mark.parametrize("kind", [V.SQUARE, V.SAW, V.TRIANGLE])
def test_moisture_with_the_other_waveforms(kind):
    """with a skew of 1 the correctly rounded power is the sample itself, and these three waveforms are the same fp32 operations on the device
    and in the restatement: the whole chain agrees bit for bit"""
    s, n, (amount, freq, _), _, _ = moisture_case(96.0, True)
    F = np.broadcast_to(np.arange(s.shape[1]), s.shape)
    got = moisture_on_device(s, n, amount, freq, 1.0, kind)
    assert np.array_equal(bits(got), bits(V.moisture(s, F, 4 * SR, SR, n, amount, freq, 1.0, kind, power32=lambda mag, k: mag)))


def test_moisture_index_clamp():
    """a synthetic n and F where Frame( t * sr ) reaches n: the kernel reads curve element n - 1, not the poisoned one behind it"""
    n, n_over = 100, 401
    idx, raw = V.curve_index(np.arange(n_over), 4 * SR, SR, n)
    assert raw[400] == n and idx[400] == n - 1
    s = np.full((1, n_over), 0.5, F32)
    amount = (np.arange(n) / n).astype(F32)
    got = moisture_on_device(s, n, amount, 3.0, 2.0, spare=4)
    want = V.moisture(s, np.arange(n_over)[None, :], 4 * SR, SR, n, amount, 3.0, 2.0)
    assert np.max(np.abs(got - want)) <= 2.0 ** -22 and abs(got[0, 400]) < 10
    assert got[0, 400] == got[0, 399] and got[0, 399] != got[0, 395]                      # both read amount[99]; frame 395 reads amount[98]


def test_cpp_add_moisture_against_the_restated_pipeline(dumped):
    """the oracle's chains around the restatement b; the bound is 2 E_ref of the case plus the half-band chains' own (the down-chain is linear with
    unit passband gain)"""
    for name, ch, n, amount, frequency, skew, kind in (("moisture_2x20001", 2, 20001, 0.5, 96.0, 4.0, V.SINE), ("moisture_low", 2, 20001, 0.5, 3.0, 4.0, V.SINE),
                                                       ("moisture_1x50", 1, 50, 0.5, 96.0, 4.0, V.SINE), ("moisture_curves", 2, 20001, None, None, None, V.SINE)):
        x = take(ch, n)
        if amount is None:
            t = [F32(f) * (F32(1.0) / F32(SR)) for f in range(n)]
            amount = np.array([F32(0.2) + v for v in t], F32)
            frequency = np.array([F32(40.0) + F32(100.0) * v for v in t], F32)
            skew = np.array([F32(2.0) + F32(3.0) * v for v in t], F32)
        up = O.resample_chain(x, SR, 4 * SR)
        F = np.broadcast_to(np.arange(up.shape[1]), up.shape)
        a = V.moisture_truth(up, F, 4 * SR, SR, n, amount, frequency, skew, kind)
        b = V.moisture(up, F, 4 * SR, SR, n, amount, frequency, skew, kind)
        e_ref = np.max(np.abs(b - a))
        want = O.resample_chain(b, 4 * SR, SR)
        got, sr = dumped[name]
        assert sr == SR and got.shape == want.shape == (ch, n)
        d = np.max(np.abs(got.astype(np.float64) - want))
        print("\n%s: E_ref %.3e  device - pipeline %.3e  bound %.3e" % (name, e_ref, d, 2 * e_ref + HB_CHAIN_BOUND))
        assert d <= 2 * e_ref + HB_CHAIN_BOUND


# ---- energies ---------------------------------------------------------------------------------------------------------------------------
def energy_on_device(x, offset=0):
    ch, n = x.shape
    keep, px = placed(x, offset)
    d_ws = fa.DeviceArray(host=np.full(fa.audio_energy_workspace_bytes(ch, n), 0xFF, np.uint8))
    out = Out(ch)
    fa.audio_energy_dev(px, ch, n, out.ptr, d_ws)
    return out.host()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 4096, 4099, 100003])
def test_total_energy_within_one_ulp(n):
    x = uniform((3, n), 41 + n)
    x[1] = 0
    for offset in (0, 1):
        got, want = energy_on_device(x, offset), V.energy_truth(x)
        assert got[1] == 0
        for c in range(3):
            assert abs(float(got[c]) - float(want[c])) <= V.ulp(want[c]), (n, c, got[c], want[c])
        assert np.array_equal(bits(got), bits(energy_on_device(x, offset)))                # the same bits on every run
    y = x.copy()
    y[0, n // 2] = 1e19                    # its square, 1e38, is still below fp32's largest value
    y[2, n - 1] = 2e19                     # 4e38 is not: inf, as an fp32 sum gives
    got, want = energy_on_device(y), V.energy_truth(y)
    assert np.isfinite(got[0]) and abs(float(got[0]) - float(want[0])) <= V.ulp(want[0]) and np.isinf(got[2]) and np.isinf(want[2]) and got[1] == 0


def test_cpp_energies(dumped):
    x = take(3, 4099)
    got, want = dumped["energy"][0][0], V.energy_truth(x)
    half, want_half = dumped["energy_half"][0][0], V.energy_truth(x - F32(0.5) * x)         # the fp32 difference signal, 0.5 x exactly
    for c in range(3):
        assert abs(float(got[c]) - float(want[c])) <= V.ulp(want[c])
        assert abs(float(half[c]) - float(want_half[c])) <= V.ulp(want_half[c])
        assert abs(float(half[c]) - 0.25 * float(want[c])) <= V.ulp(want_half[c])
    assert np.array_equal(bits(got), bits(energy_on_device(x)))


# ---- get_amplitude_envelope ----------------------------------------------------------------------------------------------------------------
def test_rectifier():
    x = uniform((2, 1003), 51)
    x[0, :4] = [0.0, -0.0, -np.inf, np.nan]
    out = Out(x.size)
    fa.audio_rectify_dev(fa.DeviceArray(host=x), 2, 1003, out.ptr)
    assert np.array_equal(bits(out.host((2, 1003))), bits(V.rectify(x)))


def test_cpp_amplitude_envelope(dumped):
    """2 ch x 3000 with a window of 480 frames at a rate of 65536, where frame times are exact and the Function hands back its own samples:
    bit for bit the composition through the C ABI, and within the convolution's bounds of the direct O( n m ) fp64 sum"""
    ys, sr = dumped["envelope"]
    ys = ys[0]
    x = take(2, 3000)
    assert sr == 65536.0 and ys.size == 3482 and np.all(ys[3479:] == 0)                    # x < size - 1: the last sample is never returned
    rect = V.rectify(V.mono(x))
    window, total = V.hann_window(F32(F32(480.0 / 65536.0) * F32(65536.0)))
    assert window.size == 480
    d_m = fa.DeviceArray(host=x)
    mono, rectified = Out(3000), Out(3000)
    fa.audio_to_mono_dev(d_m, 2, 3000, mono.ptr)
    fa.audio_rectify_dev(mono.ptr, 1, 3000, rectified.ptr)
    assert np.array_equal(bits(rectified.host()), bits(rect))
    conv = Out(3480)
    d_ws = fa.DeviceArray(host=np.full(fa.convolve_workspace_bytes(1, 3000, 1, 480), 0xFF, np.uint8))
    fa.convolve_dev(rectified.ptr, 1, 3000, fa.DeviceArray(host=window), 1, 480, 65536.0, False, conv.ptr, d_ws)
    scaled = Out(3480)
    fa.audio_gain_dev(conv.ptr, 1, 3480, float(V.envelope_gain(total)), scaled.ptr)
    composed = scaled.host()
    assert np.array_equal(bits(ys[:3479]), bits(composed[:3479]))
    truth = float(V.envelope_gain(total)) * R.truth(rect[None, :], window[None, :])
    rel_rms, rel_max = R.errors(composed[None, :], truth)
    print("\nenvelope: rel_rms %.3e rel_max %.3e (bounds %.1e, %.1e)" % (rel_rms, rel_max, R.REL_RMS_BOUND, R.REL_MAX_BOUND))
    assert rel_rms <= R.REL_RMS_BOUND and rel_max <= R.REL_MAX_BOUND
    # linear in between, at frame mid-points: the Function's own arithmetic on its samples
    assert V.envelope_function(composed, 65536.0, F32(10.5 / 65536.0)) == F32(composed[10] + F32(F32(composed[11] - composed[10]) * F32(0.5)))
