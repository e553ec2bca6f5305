"""The C ABI of flan_amd/csrc/volume.hip without a device: every entry point refuses what the header says it refuses before it looks for a
device, the size and workspace helpers, and the host-only helpers (the fade plan, the named waveforms, the white-noise draw, the oscillator's
sizes) against tests/volume_reference.py."""
import numpy as np
import pytest

import flan_amd as fa
import volume_reference as V

F32 = np.float32
BOGUS = 1 << 41                 # a pointer nobody dereferences: the checks come before any device call
FAR = BOGUS + (1 << 30)


def code(call):
    with pytest.raises(fa.FlanHipError) as e:
        call()
    return e.value.code


def passes_the_checks(call):
    """with good arguments the call gets as far as the device: it runs there, and without one it says so"""
    if fa.lib.flanhip_device_count() > 0:
        return                                  # a GPU is visible: the call would run on pointers that are not memory
    assert code(call) == fa.ERR_NO_DEVICE


def test_ring_modulate_refusals():
    good = lambda: fa.audio_ring_modulate_dev(BOGUS, 2, 100, FAR, 1, 7, BOGUS + 4096)
    assert code(lambda: fa.audio_ring_modulate_dev(None, 2, 100, FAR, 1, 7, BOGUS + 4096)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_ring_modulate_dev(BOGUS, 2, 100, None, 1, 7, BOGUS + 4096)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_ring_modulate_dev(BOGUS, 2, 100, FAR, 1, 7, None)) == fa.ERR_INVALID_ARG
    for ch, n, och, on in ((0, 100, 1, 7), (2, 0, 1, 7), (2, 100, 0, 7), (2, 100, 1, 0), (-1, 100, 1, 7), (2, 2 ** 31, 1, 7)):
        assert code(lambda: fa.audio_ring_modulate_dev(BOGUS, ch, n, FAR, och, on, BOGUS + (1 << 36))) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_ring_modulate_dev(BOGUS, 2, 100, FAR, 1, 7, BOGUS + 16)) == fa.ERR_INVALID_ARG      # a partial overlap
    assert code(lambda: fa.audio_ring_modulate_dev(BOGUS, 2, 100, BOGUS + 4096, 1, 7, BOGUS + 4096)) == fa.ERR_INVALID_ARG      # the modulator is the output
    passes_the_checks(good)


def test_fade_refusals():
    assert code(lambda: fa.audio_fade_dev(None, 2, 100, FAR, 5, FAR + 64, 5, BOGUS)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_fade_dev(BOGUS, 2, 100, None, 5, FAR + 64, 5, BOGUS)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_fade_dev(BOGUS, 2, 100, FAR, 5, None, 5, BOGUS)) == fa.ERR_INVALID_ARG
    for ch, n, s, e in ((0, 100, 5, 5), (2, 0, 0, 0), (2, 100, -1, 5), (2, 100, 5, -1), (2, 100, 101, 0), (2, 100, 0, 101)):
        assert code(lambda: fa.audio_fade_dev(BOGUS, ch, n, FAR, s, FAR + 1024, e, BOGUS)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_fade_dev(BOGUS, 2, 100, BOGUS + 8, 5, FAR, 5, BOGUS)) == fa.ERR_INVALID_ARG         # a table inside the output
    passes_the_checks(lambda: fa.audio_fade_dev(BOGUS, 2, 100, None, 0, FAR, 5, BOGUS))                                # in place, no start table


def test_fade_plan_against_the_restatement_and_by_hand():
    assert fa.fade_frames_plan(1000, 16, 16) == (16, 16)
    assert fa.fade_frames_plan(1000, -3, 7) == (0, 7) and fa.fade_frames_plan(1000, 7, -3) == (7, 0) and fa.fade_frames_plan(1000, -1, -2) == (0, 0)
    assert fa.fade_frames_plan(1000, 700, 700) == (500, 500)
    assert fa.fade_frames_plan(10, 3, 30) == (0, 9) and fa.fade_frames_plan(7, 5, 5) == (3, 3)
    assert fa.fade_frames_plan(5, 2 ** 31 - 1, 2 ** 31 - 1) == V.fade_plan(5, 2 ** 31 - 1, 2 ** 31 - 1)      # the sum is formed in 64 bits
    rng = np.random.default_rng(3)
    for _ in range(2000):
        n = int(rng.integers(1, 5000))
        s, e = (int(v) for v in rng.integers(-50, 3 * n, 2))
        got = fa.fade_frames_plan(n, s, e)
        assert got == V.fade_plan(n, s, e), (n, s, e)
        assert 0 <= got[0] <= n and 0 <= got[1] <= n
    out = np.zeros(2, np.int32)
    assert fa.lib.flanhip_fade_frames_plan(0, 1, 1, out.ctypes.data_as(fa._vp)) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_fade_frames_plan(10, 1, 1, None) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_fade_frames_plan(2 ** 31, 1, 1, out.ctypes.data_as(fa._vp)) == fa.ERR_INVALID_ARG


def test_named_waveforms_on_the_host():
    rng = np.random.default_rng(4)
    t = np.concatenate([rng.uniform(-4, 4, 4000), [0.0, 0.25, 0.5, 0.75, 1.0, -0.25, -0.5, -0.75, -1.0, 603.18, -603.18]]).astype(F32)
    for kind in (V.SQUARE, V.SAW, V.TRIANGLE):                  # the same fp32 operations: the same bits, negative t included
        assert np.array_equal(fa.waveform_host(kind, t).view(np.uint32), V.waveform(kind, t).view(np.uint32)), kind
    neg = np.array([-0.25], F32)
    assert fa.waveform_host(V.SQUARE, neg)[0] == -1 and fa.waveform_host(V.SAW, neg)[0] == -1.5 and fa.waveform_host(V.TRIANGLE, neg)[0] == -2
    # the sine: the C library's sinf at the fp32 product, within 2 ulp of a value below 1 of the sine there (2^-23); the product pi2 * t0 has
    # rounded too: half an ulp of a value below 8, 2^-22, through a slope of at most 1
    s = fa.waveform_host(V.SINE, t)
    assert np.max(np.abs(s - V.waveform_truth(V.SINE, t))) <= 2.0 ** -22 + 2.0 ** -23
    assert fa.waveform_host(V.SINE, neg)[0] < -0.999999
    assert fa.lib.flanhip_waveform_host(4, fa._ptr(t), t.size, fa._ptr(s)) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_waveform_host(-1, fa._ptr(t), t.size, fa._ptr(s)) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_waveform_host(0, None, t.size, fa._ptr(s)) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_waveform_host(0, fa._ptr(t), 0, fa._ptr(s)) == fa.ERR_INVALID_ARG


def test_waveform_dev_refusals():
    assert code(lambda: fa.waveform_dev(0, None, 10, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.waveform_dev(0, BOGUS, 10, None)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.waveform_dev(0, BOGUS, 0, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.waveform_dev(7, BOGUS, 10, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.waveform_dev(0, BOGUS, 10, BOGUS + 8)) == fa.ERR_INVALID_ARG
    passes_the_checks(lambda: fa.waveform_dev(3, BOGUS, 10, BOGUS))


def test_moisture_refusals():
    ok = dict(amount=0.5, frequency=96.0, skew=4.0, kind=0)
    call = lambda d_in=BOGUS, ch=2, n_over=400, over=192000.0, n=100, sr=48000.0, d_out=FAR, **k: fa.audio_moisture_dev(d_in, ch, n_over, over, n, sr, d_out=d_out, **dict(ok, **k))
    assert code(lambda: call(d_in=None)) == fa.ERR_INVALID_ARG and code(lambda: call(d_out=None)) == fa.ERR_INVALID_ARG
    for bad in (dict(ch=0), dict(n_over=0), dict(n=0), dict(over=0.0), dict(sr=0.0), dict(sr=-1.0), dict(kind=4), dict(kind=-1), dict(n_over=2 ** 31), dict(d_out=BOGUS + 4)):
        assert code(lambda: call(**bad)) == fa.ERR_INVALID_ARG, bad
    passes_the_checks(lambda: call(d_out=BOGUS))


def test_energy_helpers_and_refusals():
    assert fa.audio_energy_workspace_bytes(0, 10) == 0 and fa.audio_energy_workspace_bytes(1, 0) == 0 and fa.audio_energy_workspace_bytes(1, 2 ** 31) == 0
    assert fa.audio_energy_workspace_bytes(1, 1) == 256                 # one fp64 block sum, rounded up to 256 bytes
    assert fa.audio_energy_workspace_bytes(3, 100003) >= 8 * 3 * 25     # 4096 frames per block
    assert fa.audio_energy_workspace_bytes(2, 480000) % 256 == 0
    assert code(lambda: fa.audio_energy_dev(None, 1, 10, FAR, FAR + 4096)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_energy_dev(BOGUS, 1, 10, None, FAR + 4096)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_energy_dev(BOGUS, 1, 10, FAR, None)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_energy_dev(BOGUS, 0, 10, FAR, FAR + 4096)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_energy_dev(BOGUS, 1, 0, FAR, FAR + 4096)) == fa.ERR_INVALID_ARG
    passes_the_checks(lambda: fa.audio_energy_dev(BOGUS, 1, 10, FAR, FAR + 4096))


def test_rectify_refusals():
    assert code(lambda: fa.audio_rectify_dev(None, 1, 10, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_rectify_dev(BOGUS, 1, 10, None)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_rectify_dev(BOGUS, 0, 10, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_rectify_dev(BOGUS, 1, 0, FAR)) == fa.ERR_INVALID_ARG
    passes_the_checks(lambda: fa.audio_rectify_dev(BOGUS, 1, 10, BOGUS))


def test_oscillator_sizes_and_refusals():
    assert fa.synthesize_waveform_frames(0.5, 48000.0, 16) == (24000, 384000, 768000.0)
    for length, sr, over in ((0.5, 48000.0, 16), (0.1, 44100.0, 3), (1.0 / 3.0, 8000.0, 1), (2.5, 96000.0, 32)):
        assert fa.synthesize_waveform_frames(length, sr, over) == V.synthesize_waveform_frames(length, sr, over)
    for length, sr, over in ((0.5, 48000.0, 0), (0.5, 48000.0, -1), (0.0, 48000.0, 1), (-1.0, 48000.0, 1), (1.0, 0.0, 1), (1.0, -5.0, 1), (1e-9, 48000.0, 4),
                             (float("nan"), 48000.0, 1), (1e6, 48000.0, 16)):
        assert fa.synthesize_waveform_frames(length, sr, over) is None, (length, sr, over)
        assert fa.audio_synthesize_waveform_workspace_bytes(length, sr, over) == 0
        assert code(lambda: fa.audio_synthesize_waveform_dev(0, 440.0, length, sr, over, BOGUS, FAR)) == fa.ERR_INVALID_ARG
    assert fa.osc_workspace_bytes(0) == 0 and fa.osc_workspace_bytes(2 ** 31) == 0
    run, block = fa.osc_run_frames(), fa.osc_block_frames()
    assert block == 256 * run and fa.osc_carry_pass_blocks() == 256
    assert fa.osc_workspace_bytes(block) == fa.osc_workspace_bytes(1) and fa.osc_workspace_bytes(300 * block + 1) > fa.osc_workspace_bytes(block)
    with fa.osc_run_forced(1):
        assert fa.osc_run_frames() == 1 and fa.osc_block_frames() == 256
        assert fa.osc_workspace_bytes(65536 + 257) >= 2 * 16 * 258
    with fa.osc_run_forced(1000):
        assert fa.osc_run_frames() == 64
    assert fa.osc_run_frames() == run
    assert fa.audio_synthesize_waveform_workspace_bytes(0.5, 48000.0, 16) >= fa.osc_workspace_bytes(384000) + 4 * 384000
    good = lambda **k: fa.osc_phase_dev(**dict(dict(freq=440.0, n_in=1000, in_rate=768000.0, d_phases=BOGUS, d_wave=None, kind=-1, d_ws=FAR), **k))
    for bad in (dict(n_in=0), dict(n_in=2 ** 31), dict(in_rate=0.0), dict(in_rate=float("inf")), dict(d_phases=None), dict(d_ws=None), dict(d_wave=BOGUS + 8192, kind=-1),
                dict(d_wave=BOGUS + 8192, kind=4)):
        assert code(lambda: good(**bad)) == fa.ERR_INVALID_ARG, bad
    passes_the_checks(good)
    assert code(lambda: fa.audio_synthesize_waveform_dev(9, 440.0, 0.5, 48000.0, 16, BOGUS, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_synthesize_waveform_dev(0, 440.0, 0.5, 48000.0, 16, None, FAR)) == fa.ERR_INVALID_ARG
    assert code(lambda: fa.audio_synthesize_waveform_dev(0, 440.0, 0.5, 48000.0, 16, BOGUS, None)) == fa.ERR_INVALID_ARG
    passes_the_checks(lambda: fa.audio_synthesize_waveform_dev(0, 440.0, 0.5, 48000.0, 16, BOGUS, FAR))


def test_oneshot_resample_refusals():
    good = lambda **k: fa.oneshot_resample_dev(**dict(dict(d_in=BOGUS, n_in=1600, src_rate=768000.0, dst_rate=48000.0, d_out=FAR, n_out=100), **k))
    for bad in (dict(d_in=None), dict(d_out=None), dict(n_in=0), dict(n_out=0), dict(src_rate=0.0), dict(dst_rate=-1.0), dict(n_in=2 ** 31)):
        assert code(lambda: good(**bad)) == fa.ERR_INVALID_ARG, bad
    passes_the_checks(good)
    passes_the_checks(lambda: good(src_rate=48000.0))                   # equal rates are served: a copy


def test_white_noise_draw_against_the_restatement():
    for seed, count in ((0, 1), (7, 257), (2 ** 32 + 7, 257), (123456789, 1000)):
        got = fa.white_noise_draw(seed, count)
        assert np.array_equal(got.view(np.uint32), V.white_noise_draw(seed & 0xFFFFFFFF, count).view(np.uint32)), seed
    assert np.array_equal(fa.white_noise_draw(7, 64), fa.white_noise_draw(7, 300)[:64])
    assert not np.array_equal(fa.white_noise_draw(7, 64), fa.white_noise_draw(8, 64))
    out = np.zeros(4, F32)
    assert fa.lib.flanhip_white_noise_draw(1, 0, fa._ptr(out)) == fa.ERR_INVALID_ARG
    assert fa.lib.flanhip_white_noise_draw(1, 4, None) == fa.ERR_INVALID_ARG
