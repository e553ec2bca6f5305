"""tests/repitch_reference.py -- Audio::repitch restated in Python -- against the vectors the reference's own WDL_Resampler made
(tests/golden/ref_made/wdl_repitch.npz, make_wdl_repitch.py).  Plan, block count, `wanted` per block and output length exactly; the
samples bit for bit: the order of every operation is specified, and both sides call the same libm for the table.
plan() itself asserts, on every case, that each block delivers all g samples, that the 31-zero prelude is written once, and that the
resampler's buffer is a window of one continuous stream."""
import numpy as np
import pytest

import repitch_reference as R

CASES = R.load_cases()
IDS = [c["name"] for c in CASES]
RUN_CASES = R.load_cases(R.GOLDEN_RUNS)                     # the run planner's cases (wdl_repitch_runs.npz): held to the same here
RUN_IDS = [c["name"] for c in RUN_CASES]
_restated = {}


def restated(case):
    if case["name"] not in _restated:
        _restated[case["name"]] = R.repitch(case["x"], case["sr"], case["inv"], case["g"], case["quality"])
    return _restated[case["name"]]


def test_the_fixture_holds_the_cases_the_design_lists():
    assert len(CASES) == 21 and len(set(IDS)) == 21
    assert sum(c["quality"] == R.UNINTERPOLATED for c in CASES) == 4
    assert {c["x"].shape[0] for c in CASES} == {1, 2, 3} and {c["g"] for c in CASES} >= {1, 48, 5000}
    assert {c["x"].shape[1] for c in CASES} >= {1, 20, 1000}


@pytest.mark.parametrize("case", CASES + RUN_CASES, ids=IDS + RUN_IDS)
def test_plan_is_the_references(case):
    n = case["x"].shape[1]
    blocks = R.plan(n, case["sr"], case["inv"], case["g"], case["quality"])            # (asserts the three invariants)
    assert len(blocks) == case["blocks"]
    assert np.array_equal(np.array([b["wanted"] for b in blocks], np.int32), case["wanted"])
    assert R.out_frames(case["inv"], case["g"]) == case["out_frames"] == case["out"].shape[1]
    assert np.all(case["delivered"] == case["g"])                                      # the reference itself delivered every block in full
    assert [b["first_out"] for b in blocks] == [case["g"] * i for i in range(len(blocks))]


@pytest.mark.parametrize("case", CASES + RUN_CASES, ids=IDS + RUN_IDS)
def test_samples_are_bit_identical(case):
    y = restated(case)
    assert y.shape == case["out"].shape
    assert np.array_equal(y.view(np.uint32), case["out"].view(np.uint32))


def test_table_shapes_of_the_cases():
    """which table each case runs on: what the fixture was chosen to cover"""
    want = {"one_ideal1": {(1, True)}, "half_ideal2": {(2, True)}, "p8_gcd5": {(5, True)}, "two_ideal_lp": {(1, True)},
            "up1p5": {(32, False)}, "down0p7": {(32, False)}, "step": {(1, True), (32, False)}, "cd_0p9": {(32, False)}}
    for c in CASES:
        if c["name"] in want:
            got = {(b["oversize"], b["ideal"]) for b in R.plan(c["x"].shape[1], c["sr"], c["inv"], c["g"], c["quality"])}
            assert got == want[c["name"]], c["name"]
    sweep = [c for c in CASES if c["name"] == "sweep"][0]
    blocks = R.plan(4000, sweep["sr"], sweep["inv"], sweep["g"])
    assert len({b["filtpos"] for b in blocks}) > 20                                    # a new table per block while the pitch goes up
    assert min(b["ratio"] for b in blocks) < 1.0 < max(b["ratio"] for b in blocks)
    two = [c for c in CASES if c["name"] == "two_ideal_lp"][0]
    assert R.plan(1000, two["sr"], two["inv"], two["g"])[0]["filtpos"] == 1.0 / (2.0 * 1.03)


def test_table_centre_and_mirror():
    for filtpos, oversize in ((1.0, 32), (0.4, 32), (1.0, 1), (1.0, 5), (1.0, 2), (0.3, 64)):
        t = R.table(filtpos, oversize)
        assert t.size == 64 * (oversize + 1)
        assert np.array_equal(t, t[::-1])
        half = np.float64(t[: t.size // 2])
        assert abs(half[32] / max(abs(half)) - 1.0) < 1e-6 or filtpos < 1.0            # the centre tap is the largest when nothing is cut off


def test_fma_positions_stay_within_rounding_of_the_chain():
    """the device forms srcpos as fma( j, ratio, fracpos ): against the reference's chain that moves frac by a few fp64 ulps"""
    for name in ("up1p5", "down0p7", "sweep", "g5000"):
        c = [c for c in CASES if c["name"] == name][0]
        y = R.repitch(c["x"], c["sr"], c["inv"], c["g"], c["quality"], position="fma")
        rel_rms, rel_max = R.errors(y, c["out"])
        assert rel_rms <= 1e-7 and rel_max <= 1e-7, (name, rel_rms, rel_max)        # an fp32 ulp at full scale is 6e-8: a handful of samples may flip


def test_smooth_truth_agrees_with_the_table_form():
    """constant factors: the windowed sinc at the exact position against the 32-slice interpolated table (its interpolation error)"""
    for name, factor in (("up1p5", 1.5), ("down0p7", 0.7)):
        c = [c for c in CASES if c["name"] == name][0]
        t = R.smooth_truth(c["x"], c["sr"], factor, c["out"].shape[1])
        reached = c["blocks"] * c["g"]
        rel_rms, rel_max = R.errors(c["out"][:, :reached], t[:, :reached])
        print(name, rel_rms, rel_max)
        assert rel_rms < 2e-3 and rel_max < 5e-3                                       # linear interpolation between 32 slices: ~ (pi/32)^2 / 8
