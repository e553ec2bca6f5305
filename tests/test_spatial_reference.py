"""tests/spatial_reference.py -- Audio::stereo_spatialize and pan restated in Python -- against the vectors the reference's own
WDL_Resampler made (tests/golden/ref_made/wdl_spatial.npz, make_wdl_spatial.py).  Stretches, output length and the frames every block
delivers exactly; the samples bit for bit: the order of every operation is specified, and both sides call the same libm for the table
(DESIGN.md 4.20).  itd_plan() itself asserts the invariants on every case: the 15-zero prelude is written once, the buffer is a window of
one continuous stream, the first block delivers for srcpos < 14 only, the samples buffered between blocks stay within
[34 - ceil( ratio ), 34]; itd() that every window ends at least two samples before the buffer's end."""
import numpy as np
import pytest

import spatial_reference as S

F32 = np.float32
CASES = S.load_cases()
IDS = [c["name"] for c in CASES]


def case(name):
    return CASES[IDS.index(name)]


def test_the_fixture_holds_the_cases_the_design_lists():
    assert len(CASES) == 16 and len(set(IDS)) == 16
    assert {c["x"].size for c in CASES} >= {1, 20, 32, 33, 64, 100, 1000, 4000}
    assert {c["sr"] for c in CASES} == {44100.0, 48000.0}
    for name in ("n1", "n20", "n32"):
        assert case(name)["out_frames"] == 0 and case(name)["blocks"] == 1
    assert case("jump_away")["delivered"].max() > 2 * 2048                  # one block with thousands of outputs
    assert case("jump_away")["stretches"].max() > 100
    assert 0.5 < case("jump_near")["stretches"].min() < 0.502               # approaching at 342 m/s: ratio near 2
    far = case("far")
    assert far["out_frames"] > 48000 + 1000 and not np.any(far["out"][1100:])       # a second of sound travel: a long silent tail


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_stretches_length_and_plan_are_the_references(c):
    n = c["x"].size
    nout, stretches = S.itd_out_frames(n, c["sr"], c["dist"])
    assert nout == c["out_frames"] == c["out"].size
    assert np.array_equal(stretches, c["stretches"])
    blocks = S.itd_plan(n, c["sr"], stretches)                              # (asserts the invariants)
    assert len(blocks) == c["blocks"] == S.chunk_count(n)
    assert np.array_equal(np.array([b["count"] for b in blocks], np.int32), c["delivered"])
    assert blocks[0]["count"] == 14 and blocks[0]["buffered"] == 47         # the prelude: stretch 1, srcpos 0 ... 13
    # the reference never flushes: the centre of the last output's window lies at least 17 samples before the end of the padded input
    last = blocks[-1]
    reach = last["offset"] + int(last["fracpos"] + max(last["count"] - 1, 0) * last["ratio"]) + S.TAPS // 2
    assert reach <= S.PRELUDE + S.G * len(blocks) - 17


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_samples_are_bit_identical(c):
    y = S.itd(c["x"], c["sr"], c["stretches"], c["out_frames"])
    assert y.shape == c["out"].shape
    assert np.array_equal(y.view(np.uint32), c["out"].view(np.uint32))


def test_table_shapes_of_the_cases():
    """which tables each case runs on: what the fixture was chosen to cover"""
    def shapes(name):
        c = case(name)
        return [(b["oversize"], bool(b["ideal"]), b["filtpos"] < 1.0) for b in S.itd_plan(c["x"].size, c["sr"], c["stretches"])]
    assert set(shapes("receding")[1:]) == {(32, False, False)}              # ratio < 1: one table for the whole run
    approaching = case("approaching")
    blocks = S.itd_plan(2000, approaching["sr"], approaching["stretches"])
    assert len({b["filtpos"] for b in blocks[1:]}) > 50 and all(b["ratio"] > 1.0 for b in blocks[1:])       # a table per block
    fly = shapes("flyby")
    assert (32, False, True) in fly and (32, False, False) in fly           # crosses ratio 1: both kinds in one run
    still = shapes("still")
    assert still.count((1, True, False)) > 15 and (32, False, True) in still            # ratio exactly 1 in the middle: ideal, oversize 1
    plan = S.itd_plan(2000, case("still")["sr"], case("still")["stretches"])
    after_ideal = [plan[i + 1]["fracpos"] for i in range(1, len(plan) - 1) if plan[i]["ideal"]]
    assert after_ideal and all(f in (0.0, 1.0) for f in after_ideal)        # an ideal block hands on a rounded fracpos


def test_the_index_quirk_is_hit():
    """frame f reads the weight and the distance of frame int( ( f * ( 1.0f / sr ) ) * sr ): for some f that is f - 1"""
    for c in CASES:
        n, q = c["x"].size, S.read_index(c["x"].size, c["sr"])
        assert np.all((q == np.arange(n)) | (q == np.arange(n) - 1))
        print("%s: %d of %d frames read frame f - 1" % (c["name"], S.quirk_frames(n, c["sr"]), n))
    assert S.quirk_frames(1000, 48000.0) == 149 and S.quirk_frames(1000, 44100.0) == 218 and S.quirk_frames(1, 48000.0) == 0
    assert int(S.read_index(1000, 48000.0)[3]) in (2, 3)


def test_table_centre_and_mirror():
    for filtpos, oversize in ((1.0, 32), (0.4, 32), (1.0, 1), (1.0, 5), (1.0, 2), (0.3, 64)):
        t = S.table(filtpos, oversize)
        assert t.size == 32 * (oversize + 1)
        assert np.array_equal(t, t[::-1])
        half = np.float64(t[: t.size // 2])
        assert abs(half[16] / max(abs(half)) - 1.0) < 1e-6 or filtpos < 1.0            # the centre tap is the largest when nothing is cut off


def test_fma_positions_stay_within_rounding_of_the_chain():
    """the device forms srcpos as fma( j, ratio, fracpos ): against the reference's chain that moves frac by a few fp64 ulps"""
    for name in ("receding", "approaching", "flyby", "jump_away", "walk_cd"):
        c = case(name)
        y = S.itd(c["x"], c["sr"], c["stretches"], c["out_frames"], position="fma")
        rel_rms, rel_max = S.errors(y, c["out"])
        print(name, rel_rms, rel_max)
        assert rel_rms <= 1e-7 and rel_max <= 1e-7, (name, rel_rms, rel_max)        # an fp32 ulp at full scale is 6e-8: a handful of samples may flip


def test_limiter_against_a_direct_loop():
    sr, n = 48000.0, 600
    t = np.arange(n) / sr
    slow = np.stack([1.0 + 50.0 * t, 0.5 - 20.0 * t], 1).astype(F32)        # 54 m/s: under the limit
    fast = np.stack([1.0 + 900.0 * t, 0.5 + 0.0 * t], 1).astype(F32)        # 900 m/s: over it
    fast[300:] += F32(40.0)                                                  # and a jump
    top = np.finfo(F32).max
    ps = S.limit_positions(slow, top, sr)
    assert np.array_equal(ps, slow.astype(np.float64)) and np.array_equal(ps, S.limit_positions_direct(slow, top, sr))
    ps = S.limit_positions(fast, top, sr)
    assert np.array_equal(ps, S.limit_positions_direct(fast, top, sr))
    steps = S.mag(np.diff(ps, axis=0))
    assert np.all(steps <= 342.0 / sr * (1 + 1e-6)) and np.all(steps[5:] >= 342.0 / sr * (1 - 1e-6))    # held at 342 m/s
    curve = np.linspace(0.0, 100.0, n).astype(F32)                          # a limit that changes every frame
    ps = S.limit_positions(fast, curve, sr)
    assert np.array_equal(ps, S.limit_positions_direct(fast, curve, sr))
    ps = S.limit_positions(fast, 0.0, sr)                                   # a limit of 0: the source never leaves its first position
    assert np.array_equal(ps, S.limit_positions_direct(fast, 0.0, sr))
    assert np.all(ps == fast[0].astype(np.float64))
    ps = S.limit_positions(fast, -5.0, sr)                                  # the clamp's lower end
    assert np.all(ps == fast[0].astype(np.float64))


def test_ear_stage_properties():
    """the blend is all input where the source faces the ear's axis (75 degrees off the nose) and all low-pass opposite it; the gain is
    1 / distance"""
    n, sr = 64, 48000.0
    x, lp = np.ones(n, F32), np.zeros(n, F32)
    a = np.deg2rad(75.0)
    facing = (3.0 * np.cos(a), 3.0 * np.sin(a))
    left = S.ear(x, lp, sr, facing, 0.0, S.LEFT)
    assert np.allclose(left, 1.0 / 3.0, rtol=1e-5)
    behind = S.ear(x, lp, sr, (-facing[0], -facing[1]), 0.0, S.LEFT)
    assert np.all(np.abs(behind) < 1e-6)
    right = S.ear(x, lp, sr, (facing[0], -facing[1]), 0.0, S.RIGHT)          # the right ear mirrors the left one
    assert np.allclose(right, left, rtol=1e-6)
    inside = (0.0, float(F32(0.18) / F32(2)))                                # the ear's own place: atan2f( 0, 0 ) = 0 and 1 / epsilon
    assert S.ear(x, lp, sr, inside, 0.18, S.LEFT)[0] == pytest.approx(1e5 * 0.5 * (1 + np.cos(a)), rel=1e-5)


def test_whole_method_shapes():
    sr = 48000.0
    x = (0.5 * np.random.default_rng(1).standard_normal(400)).astype(F32)
    t = np.arange(400) / sr
    moving = np.stack([2.0 + 30.0 * t, 1.0 + 0.0 * t], 1).astype(F32)
    y = S.stereo_spatialize(x, sr, moving)
    assert y.shape[0] == 2 and y.shape[1] > 400 + 300                       # 2.2 m away: some 310 frames of travel behind the input
    still = S.stereo_spatialize(x, sr, np.array([2.0, 1.0], F32))
    assert still.shape == (2, 400 + 318) and not np.any(still[0, :307]) and not np.any(still[1, :318])
    assert S.stereo_spatialize(x[:32], sr, moving[:32]) is None             # the reference's zero-frame Audio
    assert S.stereo_spatialize(x[:33], sr, moving[:33]) is not None


def test_pan_and_conversions():
    x = np.random.default_rng(2).standard_normal((2, 50)).astype(F32)
    centre = S.pan(x, 0.0)
    assert np.allclose(centre, x * np.sqrt(2.0) * np.sin(np.pi / 8), rtol=1e-6)
    end = S.pan(x, -1.0)
    assert not np.any(end[0]) and np.allclose(end[1], x[1], rtol=2e-7)
    assert np.allclose(S.sine2(np.array([0.0, 0.5, 1.0], F32)), [0.0, np.sqrt(2) * np.sin(np.pi / 8), 1.0], atol=1e-7)
    assert np.array_equal(S.to_stereo(x[0])[0], (x[0] / np.sqrt(F32(2))).astype(F32))
    assert np.array_equal(S.to_mono(x), ((x[0] + x[1]) / F32(2)).astype(F32))
    c = S.combine([x[0], x[1, :20]])
    assert c.shape == (2, 50) and np.array_equal(c[1, :20], x[1, :20]) and not np.any(c[1, 20:])
    # widen is pan in the mid / side domain; mid / side is its own inverse up to rounding
    w = S.mid_side(S.pan(S.mid_side(x), 0.0))
    assert np.allclose(w, centre, rtol=1e-5, atol=1e-6)
