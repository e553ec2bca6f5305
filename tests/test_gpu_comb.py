"""Audio::filter_comb on the MI355X (flan_amd/csrc/comb.hip) against the NumPy restatement (tests/comb_reference.py) on its case table.

Bounds, derived, not measured.  The device follows the links in fp64, which is exact to ~1e-15, rounds u to fp32 once and runs the output
line in fp32, so per sample | y - y_truth | <= 5 * 2^-24 * ( | a u[n] | + | ( 1 - a ) u[p] | ) with u from the truth (one rounding each of
u[n], u[p], 1 - a, the two products and the sum, plus second order): comb_reference.output_bound.  The reference's own fp32 loop drifts
from the truth by far more (6e-7 of the input peak at k = 0.9, up to 9e-5 at k = 1), so the device is NOT bounded against it; both
distances are printed per case.  Bit for bit the device equals the model (comb_reference.comb_jump) everywhere, and the fp32 loop where
the feedback is 0 or no frame has a link."""
import ctypes

import numpy as np
import pytest
import torch

import flan_amd as fa
import comb_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
same_bits = R.same_bits


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def to_dev(v):
    return torch.from_numpy(np.array(v, F32)).to(torch.device("cuda", 0))


def param(v):
    return float(v) if np.ndim(v) == 0 else to_dev(v)


def run_dev(c, x=None, alias=False, words=False):
    """( y, the rounds the result went through ) through the _dev form -- words: ( y, rounds, whether a tile of the LDS level failed ) --, the workspace filled with 0xFF and out with NaN beforehand; alias: out is the
    input's own buffer"""
    dev = torch.device("cuda", 0)
    x = c["x"] if x is None else x
    ch, n = x.shape
    d_x = to_dev(x)
    d_out = d_x if alias else torch.full((ch, n), float("nan"), dtype=torch.float32, device=dev)
    d_ws = torch.full((fa.filter_comb_workspace_bytes(ch, n),), 0xFF, dtype=torch.uint8, device=dev)
    keep = [param(c[k]) for k in ("cutoff", "feedback", "wet_dry")]
    fa.filter_comb_dev(d_x, ch, n, c["sr"], *keep, c["invert"], d_out, d_ws)
    torch.cuda.synchronize()
    head = d_ws[:256].cpu().numpy().view(np.int32)
    return (d_out.cpu().numpy(), int(head[33])) + ((bool(head[32]),) if words else ())


def feedback_is_0(name):
    return R.CASES[name][3] == "k0"


def run(c, x=None):
    return fa.filter_comb(c["x"] if x is None else x, *R.args(c)[1:])


@pytest.mark.parametrize("name", R.IDS)
def test_against_the_truth_and_the_model(name):
    c, e = R.case(name), R.expected(name)
    y = run(c)
    assert y.shape == c["x"].shape and y.dtype == F32
    peak = np.abs(c["x"]).max()
    err = np.abs(y.astype(F64) - e["y64"])
    print("%s: device to truth %.3e of its bound; device to the fp32 loop %.3e, the fp32 loop to the truth %.3e of the input peak"
          % (name, (err / np.maximum(e["bound"], 1e-300)).max(), np.abs(y.astype(F64) - e["y32"]).max() / peak,
             np.abs(e["y32"].astype(F64) - e["y64"]).max() / peak))
    assert np.all(err <= e["bound"])
    assert same_bits(y, e["y"])                                               # the model, bit for bit
    if feedback_is_0(name) or not np.any(e["p"] >= 0):
        assert same_bits(y, e["y32"])                                         # and then the reference's own loop


def test_the_table_has_both_kinds_of_bit_identical_cases():
    assert any(feedback_is_0(n) for n in R.IDS) and any(not np.any(R.expected(n)["p"] >= 0) for n in R.IDS)


@pytest.mark.parametrize("name", R.IDS)
def test_host_and_device_forms_and_the_rounds(name):
    c, e = R.case(name), R.expected(name)
    host = run(c)
    dev, rounds = run_dev(c)                                                   # 0xFF in the workspace, NaN in out
    assert same_bits(host, dev)
    assert e["rounds"] <= rounds <= max(e["rounds"], 9)                        # the LDS level runs its rounds whether needed or not
    with fa.filter_comb_local_forced(-1):
        plain, rounds = run_dev(c)
    assert same_bits(plain, dev) and rounds == e["rounds"]                     # without it the rounds that did work are the model's
    again, _ = run_dev(c)
    assert same_bits(dev, again)                                               # two runs
    aliased, _ = run_dev(c, alias=True)
    assert same_bits(dev, aliased)                                             # out may be the audio


def test_the_lds_level_changes_no_bit():
    """off, the library's choice and forced counts; tiles that reach their level and tiles that do not (the device falls back)"""
    for name in R.IDS:
        c, e = R.case(name), R.expected(name)
        for forced in (-1, 0, 1, 3, 4, 5, 9):
            with fa.filter_comb_local_forced(forced):
                assert same_bits(run(c), e["y"]), (name, forced)
    with fa.filter_comb_local_forced(9):                                       # d = 1: a halo of 511 links is there
        y, rounds, failed = run_dev(R.case("chain"), words=True)
    assert not failed and rounds == 14 and same_bits(y, R.expected("chain")["y"])
    y, rounds, failed = run_dev(R.case("c440"), words=True)                    # the library's choice at d = 54.54: 3 rounds
    assert not failed and rounds == 8
    with fa.filter_comb_local_forced(9):                                       # 511 links of 55 frames are not: every round runs globally
        y, rounds, failed = run_dev(R.case("c440"), words=True)
    assert failed and rounds == 8 and same_bits(y, R.expected("c440")["y"])
    with fa.filter_comb_local_forced(3):                                       # curves run it only when forced
        y, rounds, failed = run_dev(R.case("forest"), words=True)              # delays of thousands of frames: not in a halo of 1024
        assert failed and rounds == 11 and same_bits(y, R.expected("forest")["y"])
        y, rounds, failed = run_dev(R.case("sweep"), words=True)               # 200 Hz and up: 7 links of 120 frames are
        assert not failed and rounds == 10 and same_bits(y, R.expected("sweep")["y"])


def test_a_channel_alone_and_among_three():
    for name in ("chain", "sweep", "forest", "c1_no_links"):
        c = R.case(name)
        assert c["x"].shape[0] == 3
        together = run(c)
        for channel in range(3):
            assert same_bits(run(c, c["x"][channel:channel + 1])[0], together[channel]), (name, channel)


def test_more_channels_than_a_thread_carries():
    c = R.case("forest")
    x = np.concatenate([c["x"]] * 3 + [c["x"][:2]])                            # 11 rows: two groups of channels
    y = run(c, x)
    want = R.expected("forest")["y"]
    for r in range(11):
        assert same_bits(y[r], want[r % 3]), r


def test_causality():
    for name in ("chain", "sweep", "forest"):
        c = R.case(name)
        m = 7001
        x = c["x"].copy()
        x[:, m:] = np.random.default_rng(5).uniform(-1, 1, x[:, m:].shape).astype(F32)
        y = run(c, x)
        want = R.expected(name)["y"]
        assert same_bits(y[:, :m], want[:, :m]) and not same_bits(y[:, m:], want[:, m:]), name


def test_a_nan_sample_reaches_its_descendants_only():
    c, e = R.case("forest"), R.expected("forest")
    m = int(np.argmax(np.bincount(e["p"][e["p"] >= 0])))
    x = c["x"].copy()
    x[1, m] = np.nan
    y = run(c, x)
    hit = R.descendants(e["p"], m)
    assert hit.sum() > 1 and not hit.all()                                     # a frame that reads a hit frame is hit itself
    assert same_bits(y[0], e["y"][0]) and same_bits(y[2], e["y"][2])
    assert same_bits(y[:, ~hit], e["y"][:, ~hit])                              # the clean twin's
    _, u32 = R.comb_fp32(x, *R.args(c)[1:])
    assert not np.isfinite(u32[1, hit]).any()                                  # where the reference's u is not finite ...
    assert not np.isfinite(y[1, hit]).any()                                    # ... neither is the device's: a * u is not, whatever a


def test_a_raised_cancel_flag_stops_the_call_before_any_launch():
    c = R.case("sweep")
    x = c["x"]
    out = np.full_like(x, 7.0)
    flag = ctypes.c_int(1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)                          # noqa: E731
    rc = fa.lib.flanhip_filter_comb(p(x), x.shape[0], x.shape[1], c["sr"], p(c["cutoff"]), 0.0, p(c["feedback"]), 0.0, p(c["wet_dry"]), 0.0, 0,
                                    p(out), ctypes.cast(ctypes.byref(flag), ctypes.c_void_p))
    assert rc == fa.ERR_CANCELLED
    torch.cuda.synchronize()
    assert np.all(out == 7.0)                                                  # nothing ran, nothing came back
    with pytest.raises(fa.FlanHipError) as e:
        fa.filter_comb(x, *R.args(c)[1:], cancel=flag)
    assert e.value.code == fa.ERR_CANCELLED
    flag.value = 0
    assert same_bits(fa.filter_comb(x, *R.args(c)[1:], cancel=flag), R.expected("sweep")["y"])
