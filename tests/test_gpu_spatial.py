"""Audio::stereo_spatialize, pan and the channel plumbing on the MI355X (flan_amd/csrc/spatial.hip) against the vectors the reference's own
WDL_Resampler made (tests/golden/ref_made/wdl_spatial.npz) and against the Python restatement (tests/spatial_reference.py).
Bounds: DESIGN.md 4.20 lists the measured values they are set from (<= 30 % above)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import spatial_reference as S

pytestmark = pytest.mark.gpu
F32 = np.float32
# head_itd against the reference-made outputs and the restatement: measured bit-identical on all 16 fixture cases and on jump_away with
# every delivered frame kept (the device's sin / cos in the table and fma( j, ratio, fracpos ) flip no sample of these), so held to that
# head_ild + falloff against the restatement (the device's atan2f / cosf against libm's): relative rms error, and max abs error / max |y|
EAR_RMS_BOUND = 1.5e-7          # measured at most 1.222e-7 (n = 33, head_width 1)
EAR_MAX_BOUND = 3.4e-7          # measured at most 2.641e-7 (n = 4097, head_width 0)
# the whole method against the restatement: the same two functions, then the resampler's taps
METHOD_RMS_BOUND = 2.7e-7       # measured at most 2.082e-7 (random shape 8: jumps, n = 55, head_width 1)
METHOD_MAX_BOUND = 4.8e-7       # measured at most 3.707e-7 (the same shape)

CASES = S.load_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def case(name):
    return CASES[IDS.index(name)]


def ulps(a, b):
    """the largest distance of two float32 arrays in units in the last place (same signs or zeros)"""
    a, b = np.asarray(a, F32).view(np.int32).astype(np.int64), np.asarray(b, F32).view(np.int32).astype(np.int64)
    return int(np.max(np.abs(a - b))) if a.size else 0


def itd_dev(x, sr, stretches, out_frames, stride):
    """the device form on a workspace of 0xFF and an output of NaN"""
    dev = torch.device("cuda", 0)
    x = np.atleast_2d(x)
    ears, n = x.shape
    d_x = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    d_out = torch.full((ears, stride), float("nan"), dtype=torch.float32, device=dev)
    d_ws = torch.full((fa.spatial_itd_workspace_bytes(n, sr, stretches),), 0xFF, dtype=torch.uint8, device=dev)
    fa.spatial_itd_dev(d_x, ears, n, sr, stretches, out_frames, stride, d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_itd_against_the_reference_made_output(c):
    nout, n = c["out_frames"], c["x"].size
    stride = max(nout, 1)
    y = fa.spatial_itd(c["x"], c["sr"], c["stretches"], nout, stride)
    assert y.shape == (1, stride)
    rel_rms, rel_max = S.errors(y[0, :nout], c["out"])
    differ = int(np.sum(y[0, :nout].view(np.uint32) != c["out"].view(np.uint32)))
    print("%s: rel_rms=%.3e rel_max=%.3e, %d of %d samples differ" % (c["name"], rel_rms, rel_max, differ, nout))
    assert differ == 0
    assert not np.any(y[0, min(int(c["delivered"].sum()), nout):])         # what no block reaches stays 0, and so does the row's padding
    # the device form, on a workspace that was not cleared; twice
    a, b = itd_dev(c["x"], c["sr"], c["stretches"], nout, stride), itd_dev(c["x"], c["sr"], c["stretches"], nout, stride)
    assert np.array_equal(a.view(np.uint32), y.view(np.uint32)) and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_both_ears_in_one_launch_equal_each_ear_alone():
    for left, right in (("receding", "approaching"), ("still", "receding"), ("flyby", "walk_4000")):
        l, r = case(left), case(right)
        x = np.stack([l["x"], r["x"]])
        stretches = np.stack([l["stretches"], r["stretches"]])
        nout = [l["out_frames"], r["out_frames"]]
        stride = max(nout) + 3                                              # padding behind the longer ear too
        both = fa.spatial_itd(x, l["sr"], stretches, nout, stride)
        for k, c in enumerate((l, r)):
            alone = fa.spatial_itd(c["x"], c["sr"], c["stretches"], nout[k], stride)
            assert np.array_equal(both[k].view(np.uint32), alone[0].view(np.uint32)), (left, right, k)
            assert not np.any(both[k, nout[k]:])
        dev = itd_dev(x, l["sr"], stretches, nout, stride)
        assert np.array_equal(dev.view(np.uint32), both.view(np.uint32))


def test_a_block_of_thousands_of_outputs_is_cut_into_runs():
    """jump_away: one block delivers 5054 frames, more than a run holds.  The method drops most of them; kept here, against the
    restatement"""
    c = case("jump_away")
    total = int(c["delivered"].sum())
    assert c["delivered"].max() > 2 * 2048 and total > c["out_frames"]
    want = S.itd(c["x"], c["sr"], c["stretches"], total, position="fma")
    y = fa.spatial_itd(c["x"], c["sr"], c["stretches"], total, total + 5)
    rel_rms, rel_max = S.errors(y[0, :total], want)
    print("jump_away, every delivered frame kept: rel_rms=%.3e rel_max=%.3e" % (rel_rms, rel_max))
    assert np.array_equal(y[0, :total].view(np.uint32), want.view(np.uint32))
    assert not np.any(y[0, total:])
    cut = fa.spatial_itd(c["x"], c["sr"], c["stretches"], 3000, total + 5)    # a length that ends inside the second run of the block
    assert np.array_equal(cut[0, :3000].view(np.uint32), y[0, :3000].view(np.uint32)) and not np.any(cut[0, 3000:])


# ---- head_ild + falloff ---------------------------------------------------------------------------------------------------------------------
def path(kind, n, sr, rng):
    t = np.arange(n) / sr
    if kind == "orbit":
        r, hz, ph = rng.uniform(0.5, 4.0), rng.uniform(1.0, 40.0), rng.uniform(0, 6.28)
        return np.stack([r * np.cos(2 * np.pi * hz * t + ph), r * np.sin(2 * np.pi * hz * t + ph)], 1).astype(F32)
    if kind == "walk":
        return (rng.uniform(-2, 2, 2) + np.cumsum(rng.uniform(1e-4, 3e-3) * rng.standard_normal((n, 2)), 0)).astype(F32)
    p = np.tile(rng.uniform(-3, 3, 2), (n, 1))                              # jumps: the limiter turns each into a run at 342 m/s
    for at in sorted(rng.integers(1, max(n, 2), 3)):
        p[at:] = rng.uniform(-30, 30, 2)
    return p.astype(F32)


@pytest.mark.parametrize("n", [1, 33, 1000, 4097])
@pytest.mark.parametrize("head_width", [0.0, 0.18, 1.0])
def test_ear_stage_against_the_restatement(n, head_width):
    sr = 48000.0
    rng = np.random.default_rng(n)
    x, lp = (0.5 * rng.standard_normal(n)).astype(F32), (0.3 * rng.standard_normal(n)).astype(F32)
    worst = [0.0, 0.0]
    for kind in ("orbit", "walk", "jumps", "constant"):
        ps = np.array([1.5, -0.7]) if kind == "constant" else S.limit_positions(path(kind, n, sr, rng), np.finfo(F32).max, sr)
        both = fa.spatial_ear(x, lp, sr, ps, head_width, fa.SPATIAL_BOTH)
        assert both.shape == (2, n)
        for k, (left, which) in enumerate(((S.LEFT, fa.SPATIAL_LEFT), (S.RIGHT, fa.SPATIAL_RIGHT))):
            alone = fa.spatial_ear(x, lp, sr, ps, head_width, which)
            assert np.array_equal(alone[0].view(np.uint32), both[k].view(np.uint32)), (kind, k)
            rel_rms, rel_max = S.errors(both[k], S.ear(x, lp, sr, ps, head_width, left))
            worst = [max(worst[0], rel_rms), max(worst[1], rel_max)]
    print("ear n=%d head_width=%g: worst rel_rms=%.3e rel_max=%.3e; %d frames read frame f - 1" % (n, head_width, worst[0], worst[1], S.quirk_frames(n, sr)))
    assert worst[0] <= EAR_RMS_BOUND and worst[1] <= EAR_MAX_BOUND, worst


def test_ear_stage_reads_the_geometry_of_the_frame_the_reference_reads():
    """a source that jumps every frame between two places: a frame that read its own geometry where the reference reads frame f - 1 is
    far off, not an ulp"""
    n, sr = 1000, 48000.0
    assert S.quirk_frames(n, sr) > 100
    ps = np.where((np.arange(n) % 2 == 0)[:, None], np.array([0.5, 0.2]), np.array([-4.0, 3.0])).astype(np.float64)
    x = np.ones(n, F32)
    y = fa.spatial_ear(x, np.zeros(n, F32), sr, ps, 0.18, fa.SPATIAL_LEFT)[0]
    want = S.ear(x, np.zeros(n, F32), sr, ps, 0.18, S.LEFT)
    rel_rms, rel_max = S.errors(y, want)
    assert rel_max <= EAR_MAX_BOUND, rel_max


# ---- the whole method -------------------------------------------------------------------------------------------------------------------------
def method(x, sr, positions, head_width, speed_limit):
    """stereo_spatialize composed of the C ABI's host forms as the C++ method composes it (tests/cpp/spatial_test.cpp holds the method
    itself to this, bit for bit); also returns the low-pass it ran on"""
    n = x.size
    lp = fa.filter_1pole(x[None, :], sr, 500.0, fa.FILTER_BUTTERWORTH_LOW, 1)[0]
    if np.ndim(positions) == 1:
        ps = np.asarray(positions, F32).astype(np.float64)
        shaped = fa.spatial_ear(x, lp, sr, ps, head_width)
        dev = torch.device("cuda", 0)
        delays, frames = [], []
        for left in (S.LEFT, S.RIGHT):
            dist = F32(S.mag(S.relative(ps, head_width, left))[0])
            delays.append(F32(F32(dist / S.SOUND) * F32(sr)))
            frames.append(int(F32(F32(n) + delays[-1])))
        d_out = torch.full((2, max(frames)), float("nan"), dtype=torch.float32, device=dev)
        d_shaped = torch.from_numpy(shaped).to(dev)
        fa.spatial_delay_dev(d_shaped, 2, n, delays, frames, max(frames), d_out)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), lp
    ps = S.limit_positions(positions, speed_limit, sr)
    shaped = fa.spatial_ear(x, lp, sr, ps, head_width)
    nout, stretches = zip(*(fa.spatial_itd_out_frames(n, sr, S.mag(S.relative(ps, head_width, left)[::S.G])) for left in (S.LEFT, S.RIGHT)))
    if max(nout) == 0:
        return None, lp
    return fa.spatial_itd(shaped, sr, np.stack(stretches), list(nout)), lp


def test_constant_position_is_a_pure_delay():
    sr = 48000.0
    for n, p, hw in ((1, (2.0, 1.0), 0.18), (1025, (0.3, -0.2), 0.18), (3000, (343.0, 0.0), 1.0), (500, (0.0, 0.0), 0.0)):
        x = (0.5 * np.random.default_rng(n).standard_normal(n)).astype(F32)
        y, lp = method(x, sr, np.array(p, F32), hw, None)
        want = S.stereo_spatialize(x, sr, np.array(p, F32), hw, lp=lp)
        assert y.shape == want.shape, (n, p)
        rel_rms, rel_max = S.errors(y, want)
        print("constant n=%d p=%s: %d frames rel_rms=%.3e rel_max=%.3e" % (n, p, y.shape[1], rel_rms, rel_max))
        assert np.array_equal(y == 0, want == 0) or hw == 0.0               # the same frames are written
        assert rel_rms <= METHOD_RMS_BOUND and rel_max <= METHOD_MAX_BOUND


def random_case(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(33, 5001))
    sr = float(rng.choice([44100.0, 48000.0]))
    kind = ("walk", "orbit", "jumps")[seed % 3]
    head_width = (0.0, 0.18, 1.0)[(seed // 3) % 3]
    limit = np.finfo(F32).max if seed % 4 else rng.uniform(0.0, 60.0, n).astype(F32)
    x = (0.5 * rng.standard_normal(n)).astype(F32)
    return x, sr, path(kind, n, sr, rng), head_width, limit, kind


def test_random_shapes_against_the_restatement():
    worst = [0.0, 0.0]
    for seed in range(20):
        x, sr, positions, head_width, limit, kind = random_case(seed)
        y, lp = method(x, sr, positions, head_width, limit)
        want = S.stereo_spatialize(x, sr, positions, head_width, limit, lp=lp)
        assert y.shape == want.shape, seed
        rel_rms, rel_max = S.errors(y, want)
        print("seed %d: %s n=%d sr=%g head_width=%g -> %d frames  rel_rms=%.3e rel_max=%.3e" % (seed, kind, x.size, sr, head_width, y.shape[1], rel_rms, rel_max))
        worst = [max(worst[0], rel_rms), max(worst[1], rel_max)]
    print("worst rel_rms=%.3e rel_max=%.3e" % tuple(worst))
    assert worst[0] <= METHOD_RMS_BOUND and worst[1] <= METHOD_MAX_BOUND, worst


def test_short_inputs_have_no_output_frames():
    sr = 48000.0
    for n in (1, 20, 32):
        x = np.ones(n, F32)
        y, _ = method(x, sr, path("walk", n, sr, np.random.default_rng(n)), 0.18, np.finfo(F32).max)
        assert y is None and S.stereo_spatialize(x, sr, path("walk", n, sr, np.random.default_rng(n))) is None


# ---- pan, the conversions, the channel copies ---------------------------------------------------------------------------------------------
LENGTHS = (1, 3, 4, 5, 1023, 1025)


def on_device(a, offset):
    """`a` on the device `offset` floats behind a 16-byte boundary (torch allocations are aligned far beyond that)"""
    dev = torch.device("cuda", 0)
    base = torch.full((a.size + offset + 8,), float("nan"), dtype=torch.float32, device=dev)
    view = base[offset:offset + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return base, view


@pytest.mark.parametrize("n", LENGTHS)
def test_pan(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal((2, n)).astype(F32)
    curve = rng.uniform(-1, 1, n).astype(F32)
    for amount in (curve, 0.3, -1.0, 1.0):
        want = S.pan(x, amount)
        y = fa.audio_pan(x, amount)
        assert ulps(y, want) <= 1, (n, ulps(y, want))
        for off_in, off_out, off_pan in ((0, 0, 0), (1, 3, 2), (3, 0, 1), (0, 1, 0)):
            (_, d_x), (base, d_y) = on_device(x, off_in), on_device(np.zeros_like(x), off_out)
            d_p = amount if np.isscalar(amount) else on_device(curve, off_pan)[1]
            fa.audio_pan_dev(d_x, 2, n, d_p, d_y)
            torch.cuda.synchronize()
            assert np.array_equal(d_y.cpu().numpy().reshape(2, n).view(np.uint32), y.view(np.uint32))
            rest = base.cpu().numpy()
            assert np.all(np.isnan(rest[:off_out])) and np.all(np.isnan(rest[off_out + 2 * n:]))      # nothing outside the output
    (_, d_x) = on_device(x, 0)                                              # in place
    fa.audio_pan_dev(d_x, 2, n, 0.3, d_x)
    torch.cuda.synchronize()
    assert np.array_equal(d_x.cpu().numpy().reshape(2, n).view(np.uint32), fa.audio_pan(x, 0.3).view(np.uint32))


@pytest.mark.parametrize("n", LENGTHS)
def test_conversions_and_channel_copies(n):
    rng = np.random.default_rng(10 + n)
    x = rng.standard_normal((3, n)).astype(F32)
    for off_in, off_out in ((0, 0), (1, 3), (3, 0), (2, 2)):
        (_, d_x) = on_device(x, off_in)
        base, d_y = on_device(np.zeros((2, n), F32), off_out)
        fa.audio_to_stereo_dev(d_x, n, d_y)                                 # channel 0 of x as a mono input
        torch.cuda.synchronize()
        assert np.array_equal(d_y.cpu().numpy().reshape(2, n).view(np.uint32), S.to_stereo(x[0]).view(np.uint32))
        rest = base.cpu().numpy()
        assert np.all(np.isnan(rest[:off_out])) and np.all(np.isnan(rest[off_out + 2 * n:]))
        for ch in (1, 2, 3):
            base, d_m = on_device(np.zeros(n, F32), off_out)
            fa.audio_to_mono_dev(d_x, ch, n, d_m) if ch == 3 else fa.audio_to_mono_dev(on_device(x[:ch], off_in)[1], ch, n, d_m)
            torch.cuda.synchronize()
            assert np.array_equal(d_m.cpu().numpy().view(np.uint32), S.to_mono(x[:ch]).view(np.uint32))
            rest = base.cpu().numpy()
            assert np.all(np.isnan(rest[:off_out])) and np.all(np.isnan(rest[off_out + n:]))
        # combine: the three rows into rows 1 ... 3 of a five-row output seven frames longer; what lies behind them is zero
        longer = n + 7
        base, d_c = on_device(np.full((5, longer), 9.0, F32), off_out)
        fa.audio_copy_rows_dev(d_x, n, 3, n, d_c[longer:], longer, longer)
        torch.cuda.synchronize()
        got = d_c.cpu().numpy().reshape(5, longer)
        assert np.array_equal(got[1:4, :n].view(np.uint32), x.view(np.uint32)) and not np.any(got[1:4, n:])
        assert np.all(got[0] == 9.0) and np.all(got[4] == 9.0)
        rest = base.cpu().numpy()
        assert np.all(np.isnan(rest[:off_out])) and np.all(np.isnan(rest[off_out + 5 * longer:]))
        # split: row 2 into a buffer of its own
        base, d_s = on_device(np.zeros(n, F32), off_out)
        fa.audio_copy_rows_dev(d_x[2 * n:], n, 1, n, d_s, n, n)
        torch.cuda.synchronize()
        assert np.array_equal(d_s.cpu().numpy().view(np.uint32), x[2].view(np.uint32))
        rest = base.cpu().numpy()
        assert np.all(np.isnan(rest[:off_out])) and np.all(np.isnan(rest[off_out + n:]))
