"""The YIN pitch tracker on the MI355X (flan_amd/csrc/pitch.hip) against the fp64 truth and the NumPy restatement (tests/pitch_reference.py).

The reference cannot be built for this family, so the truth is d as its definition in fp64, and the reference's own noise is measured on a
stand-in: compute_d restated in fp32 around a single precision FFT.  Tones lie over a noise floor: on an exactly periodic signal the lowest
valley's y is 0 up to rounding and the reference answers 0 or the period by the sign of that noise (kept; pinned on crafted rows instead).

  d'        max | d'_gpu - d'_truth | <= 4 x max | d'_standin - d'_truth | per case, the right side computed here on the same input and
            printed.  4: an FFT path on the device would carry the reference's kind of error in another order.  Zeros and DC: d' == 1
  pick      every output bit equals the restatement's, on the truth's d' rows and on the crafted rows
  fused     the one-launch form equals dprime -> pick, bit for bit
  end to end  a window is left out only where the stand-in itself disagrees with the truth (one zero and the other not, or more than 1e-3
            apart), at most 2 % of a case; elsewhere zero and non-zero agree and | w - w_truth | <= max( 4 E, 2^-22 ) w, E the stand-in's
            largest relative deviation over the six signals and four larger shapes, measured here; 2^-22: two fp32 spacings of x"""
import ctypes
import os

import numpy as np
import pytest
import torch

import flan_amd as fa
import host_cpp
import pitch_reference as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
SR = R.SR
CASES = [(s, k) for s in R.SIGNALS for k in R.SHAPES]
CLEAN = [(s, k) for s in ("zeros", "dc") for k in R.SHAPES]
DEV = torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def to_dev(v):
    return torch.from_numpy(np.array(v, F32)).to(DEV)


def filled(shape, value=float("nan")):
    return torch.full(shape, value, dtype=torch.float32, device=DEV)


def geometry(shape):
    window, hop, frames, start, end = R.SHAPES[shape]
    return window, hop, frames, start, end, R.count(frames, start, end, window, hop), window // 2


def dev_dprime(x, shape):
    window, hop, frames, start, end, count, h = geometry(shape)
    d_x, d_out = to_dev(x), filled((count, h))
    fa.yin_dprime_dev(d_x, frames, start, end, window, hop, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def dev_pick(rows, cutoff=0.2, minimum=10):
    rows = np.atleast_2d(np.ascontiguousarray(rows, F32))
    d_rows, d_out = to_dev(rows), filled((rows.shape[0],))
    fa.yin_pick_dev(d_rows, rows.shape[0], rows.shape[1], cutoff, minimum, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def dev_fused(x, shape, cutoff=0.2, minimum=10):
    window, hop, frames, start, end, count, h = geometry(shape)
    d_x, d_out = to_dev(x), filled((count,))
    d_ws = torch.full((fa.local_wavelengths_workspace_bytes(frames, start, end, window, hop),), 0xFF, dtype=torch.uint8, device=DEV)
    fa.local_wavelengths_dev(d_x, frames, start, end, window, hop, cutoff, minimum, d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def host_form(x, shape):
    window, hop, frames, start, end, count, h = geometry(shape)
    return fa.local_wavelengths(x, SR, start, end, window, hop)


@pytest.fixture(scope="module")
def suite_E():
    """the stand-in's largest relative deviation from the truth over the six signals and the four larger shapes, and how many windows it
    disagrees on: decided without the code under test"""
    E, out, windows = 0.0, 0, 0
    for name in R.SIGNALS:
        for shape in R.LARGER:
            t = R.truth(name, shape)
            excluded, rel = R.disagreement(t["raw_standin"], t["raw"])
            E = max(E, float(rel[~excluded].max()) if np.any(~excluded) else 0.0)
            out += int(excluded.sum())
            windows += excluded.size
    print("stand-in: disagrees on %d of %d windows, largest relative deviation elsewhere %.3e" % (out, windows, E))
    return E


# ---- 1: d' ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES)
def test_dprime_against_the_truth(name, shape):
    t = R.truth(name, shape)
    got = dev_dprime(t["x"], shape)
    assert got.shape == t["dprime"].shape and got.dtype == F32 and np.all(np.isfinite(got))
    mine = np.abs(got.astype(F64) - t["dprime"].astype(F64)).max()
    theirs = np.abs(t["dprime_standin"].astype(F64) - t["dprime"].astype(F64)).max()
    print("%s %s: max |d' - truth| device %.3e, stand-in %.3e; rows equal to the truth's bit for bit: %d of %d"
          % (name, shape, mine, theirs, int(np.sum(np.all(got.view(np.uint32) == t["dprime"].view(np.uint32), axis=1))), got.shape[0]))
    assert mine <= 4 * theirs
    assert np.all(got[:, 0] == 1)


@pytest.mark.parametrize("name,shape", CLEAN)
def test_silence_and_dc_give_ones(name, shape):
    window, hop, frames, start, end, count, h = geometry(shape)
    got = dev_dprime(R.signal(name, frames), shape)
    assert got.shape == (count, h) and np.all(got.view(np.uint32) == F32(1).view(np.uint32))
    assert np.all(dev_fused(R.signal(name, frames), shape).view(np.uint32) == 0)          # +0: every walk ends at an edge
    assert np.all(host_form(R.signal(name, frames), shape).view(np.uint32) == 0)


# ---- 2: the pick ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES)
def test_pick_is_the_restatement_s_bit_for_bit(name, shape):
    t = R.truth(name, shape)
    assert R.same_bits(dev_pick(t["dprime"]), t["raw"])
    for cutoff, minimum in ((0.5, 3), (1.5, 40), (0.05, 0)):
        want = np.array([R.pick(row, cutoff, minimum) for row in t["dprime"]], F32)
        assert R.same_bits(dev_pick(t["dprime"], cutoff, minimum), want), (cutoff, minimum)


@pytest.mark.parametrize("row", sorted(R.PICK_ROWS))
def test_pick_on_the_crafted_rows(row):
    values, cutoff, minimum, want = R.PICK_ROWS[row]
    got = dev_pick(values, cutoff, minimum)
    assert R.same_bits(got, [R.pick(values, cutoff, minimum)])
    if want is not None:
        assert got[0] == F32(want)
    # the same row among others, and behind padding that makes it longer than a block has threads
    if np.all(np.isfinite(values)):
        long = np.concatenate([np.full(700, 2, F32), values])                  # a flat stretch from the left edge, then the row
        assert R.same_bits(dev_pick(long, cutoff, minimum + 700), [R.pick(long, cutoff, minimum + 700)])


def test_pick_on_long_rows_with_plateaus():
    rng = np.random.default_rng(21)
    rows = np.stack([(rng.integers(0, levels, 8192) / F32(levels)).astype(F32) for levels in (2, 3, 7, 40)]
                    + [rng.uniform(0, 2, 8192).astype(F32), np.ones(8192, F32), np.where(np.arange(8192) < 4000, F32(.5), F32(.25))])
    rows[4, 5000:5400] = rows[4].min() / 2                                     # one long plateau below everything else
    for cutoff, minimum in ((0.2, 10), (1.5, 300)):
        want = np.array([R.pick(row, cutoff, minimum) for row in rows], F32)
        assert R.same_bits(dev_pick(rows, cutoff, minimum), want)
    assert F32((4999 + 5400) * 0.5) in R.valleys(rows[4])[0]                   # the plateau is one valley, at its middle


# ---- 3: fused equals split --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,shape", CASES + CLEAN)
def test_fused_equals_split(name, shape):
    window, hop, frames, start, end, count, h = geometry(shape)
    x = R.signal(name, frames)
    for cutoff, minimum in ((0.2, 10), (0.6, 2)):
        split = dev_pick(dev_dprime(x, shape), cutoff, minimum)
        fused = dev_fused(x, shape, cutoff, minimum)
        assert fused.shape == (count,) and R.same_bits(fused, split), (cutoff, minimum)
        assert R.same_bits(dev_fused(x, shape, cutoff, minimum), fused)        # two runs
    starts = R.window_starts(frames, start, end, window, hop)
    one = filled((1,))
    for w in (0, count // 2, count - 1):                                       # one window through the single-window entry point
        fa.local_wavelength_dev(to_dev(x[starts[w]:starts[w] + window]), window, 0.6, 2, one)
        torch.cuda.synchronize()
        assert R.same_bits(one.cpu().numpy(), fused[w:w + 1])


# ---- 4: end to end ----------------------------------------------------------------------------------------------------------------

def agreement(got, t, hop, E, what):
    """got against the truth's wavelengths under the rule of the module's docstring"""
    standin = R.continuity(t["raw_standin"], SR, hop)
    excluded = R.disagreement(t["raw_standin"], t["raw"])[0] | R.disagreement(standin, t["wavelengths"])[0]
    assert excluded.sum() <= 0.02 * excluded.size, what
    want = t["wavelengths"].astype(F64)
    got = got.astype(F64)
    keep = ~excluded
    assert np.array_equal(got[keep] == 0, want[keep] == 0), what
    bound = max(4 * E, 2.0 ** -22) * want
    found = keep & (want != 0)
    worst = float((np.abs(got - want)[found] / want[found]).max()) if np.any(found) else 0.0
    print("%s: %d of %d windows left out, %d found, largest relative deviation %.3e (bound %.3e)"
          % (what, int(excluded.sum()), excluded.size, int(np.sum(want != 0)), worst, max(4 * E, 2.0 ** -22)))
    assert np.all(np.abs(got - want)[keep] <= bound[keep]), what


@pytest.mark.parametrize("name,shape", CASES)
def test_host_form_end_to_end(name, shape, suite_E):
    t = R.truth(name, shape)
    hop = R.SHAPES[shape][1]
    got = host_form(t["x"], shape)
    assert got.dtype == F32 and got.shape == t["wavelengths"].shape
    agreement(got, t, hop, suite_E, "%s %s" % (name, shape))
    assert R.same_bits(got, R.continuity(dev_fused(t["x"], shape), SR, hop))   # the host form is the raw values through the continuity pass


def test_the_suite_takes_every_branch():
    branches = [b for name in R.SIGNALS for shape in R.LARGER for b in R.truth(name, shape)["branches"]]
    assert any(b == "lowest" for b in branches) and any(b == "earlier" for b in branches)
    assert any(b.endswith("+cutoff") for b in R.truth("noise", "default")["branches"])
    assert any(w != 0 for name in R.SIGNALS for w in R.truth(name, "default")["wavelengths"])


def test_a_raised_cancel_flag_stops_the_host_form():
    x = R.signal("tone220", 16000)
    flag = ctypes.c_int(1)
    with pytest.raises(fa.FlanHipError) as e:
        fa.local_wavelengths(x, SR, cancel=flag)
    assert e.value.code == fa.ERR_CANCELLED
    flag.value = 0
    assert R.same_bits(fa.local_wavelengths(x, SR, cancel=flag), fa.local_wavelengths(x, SR))


# ---- 4 and 5: the C++ methods -----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def methods(tmp_path_factory):
    """what the C++ methods answer for the glide at the default shape (tests/cpp/pitch_test.cpp --dump)"""
    host_cpp.build("pitch_test")
    folder = tmp_path_factory.mktemp("pitch")
    source, answers = os.path.join(folder, "glide.f32"), os.path.join(folder, "answers.txt")
    R.signal("glide", 16000).tofile(source)
    host_cpp.run("pitch_test", "--dump", source, answers)
    out = {}
    for line in open(answers):
        name, *values = line.split()
        out[name] = np.array([float(v) for v in values], F64).astype(F32)
    return out


def test_cpp_wavelengths_end_to_end(methods, suite_E):
    t = R.truth("glide", "default")
    agreement(methods["wavelengths"], t, 128, suite_E, "Audio::get_local_wavelengths, glide default")
    assert R.same_bits(methods["wavelengths"], host_form(t["x"], "default"))   # and the C ABI's host form, bit for bit
    # one window: the raw value of that window, and the last window that fits in the signal (which the hops never reach)
    raw = dev_fused(t["x"], "default")
    single = methods["single"]
    assert R.same_bits(single[[0, 2]], raw[[0, 5]])
    last = R.pick(R.dprime(R.d_truth(t["x"][16000 - 2048:])))
    assert last != 0 and abs(float(single[4]) - float(last)) <= max(4 * suite_E, 2.0 ** -22) * float(last)
    with np.errstate(divide="ignore"):
        assert R.same_bits(single[1::2], F32(SR) / single[0::2])               # get_local_frequency: the rate over the wavelength, inf for 0


def test_cpp_frequencies_envelope_and_average(methods, suite_E):
    t = R.truth("glide", "default")
    w, f = methods["wavelengths"], methods["frequencies"]
    want = w.copy()
    want[w != 0] = F32(SR) / w[w != 0]
    assert R.same_bits(f, want)                                                # sr / w, zeros kept
    # the envelope at 50 times: the interpolation of the returned frequencies bit for bit, and of the truth's within the end-to-end bound
    times, values = methods["times"], methods["envelope"]
    assert times.size == 50 and values.size == 50
    tol = max(4 * suite_E, 2.0 ** -22) + 2.0 ** -22                           # the wavelength's bound, the division and the interpolation
    f_truth = np.where(t["wavelengths"] != 0, SR / np.maximum(t["wavelengths"].astype(F64), 1e-300), 0.0)
    excluded = R.disagreement(t["raw_standin"], t["raw"])[0] | R.disagreement(R.continuity(t["raw_standin"], SR, 128), t["wavelengths"])[0]
    inside = 0
    for time, value in zip(times, values):
        x = F32(F32(time * F32(SR)) / F32(128))
        if not (0 <= x and x < F32(f.size - 1)):
            assert value == 0
            continue
        inside += 1
        x1 = int(np.floor(x))
        assert value == F32(f[x1] + F32(F32(f[x1 + 1] - f[x1]) * F32(x - F32(x1))))
        if excluded[x1] or excluded[x1 + 1]:
            continue
        exact = f_truth[x1] + (f_truth[x1 + 1] - f_truth[x1]) * (float(x) - x1)
        assert abs(float(value) - exact) <= tol * max(f_truth[x1], f_truth[x1 + 1]), time
    assert inside >= 45 and inside < 50                                        # some of the times lie behind the last hop
    # the averages: the restatement applied to the returned vector, bit for bit
    average = methods["average"]
    assert R.same_bits(average, [R.average(w), R.average(w), R.average(w, 0.0, 1.0)])
    assert average[0] > 0 and average[2] == -1                                 # a glide's wavelengths vary by more than a frame
