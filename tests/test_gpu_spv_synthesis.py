"""SPV::convert_to_audio on the MI355X (k_spv_chain_sums -> k_spv_scan -> k_spv_synthesize, flan_amd/csrc/spv.hip) against the numpy
restatement of the reference and its fp64 truth (tests/spv_reference.py: synthesize_np, synthesis_truth).  Nothing here needs oracle/_ref.
The SPVs of the case table are built in numpy (R.SYN_CASES); the pipeline cases take theirs from the device analysis.  Errors are
rms( d ) / rms( reference ) and max | d | / max | reference |.  Bounds: DESIGN.md 4.11 lists the measured values they are set from
(<= 30 % above)."""
import contextlib

import numpy as np
import pytest
import torch

import flan_amd as fa
import spv_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SR = 48000.0
# Against the fp64 truth: the device's two errors may be at most TRUTH_FACTOR times synthesize_np's own on the same case.  The device
# sums the bins in another order (per-thread partials, two LDS stages) and takes its cosine from sincos_fast (7e-8 absolute); nothing
# else may differ.  From 256 bins up the device is 2 to 10 times CLOSER to the truth than the bin-order sum (ratios 0.09 .. 0.47); the
# ratios above 1 all come from the cases of 2 to 7 bins, where either error is one or two fp32 ulps of the output.
TRUTH_FACTOR = 2.48            # measured on the MI355X at most 1.91 (one_chain_N7_n33, max / peak: 6.10e-8 against 3.20e-8); rms 1.25 (same case)
# Against the restatement, per regime of f: (rel rms, max / peak), each <= 30 % above the largest value measured on the MI355X
REST_BOUND = {
    "uniform": (1.54e-6, 2.09e-6),       # measured 1.187e-6, 1.611e-6 (both bins4097: the bin-order sum's own error grows with sqrt( N ))
    "negative": (4.40e-7, 5.84e-7),      # measured 3.388e-7, 4.497e-7 (negative, under every cut)
    "wide": (5.80e-7, 1.32e-6),          # measured 4.462e-7 (pipeline N=513 set_440.5), 1.019e-6 (pipeline N=513 as_is)
    "extreme": (1.28e-7, 2.41e-7),       # measured 9.895e-8, 1.857e-7 (both sincos_wide; fold_any 9.36e-8, 1.30e-7)
}


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def cut_of(cut):
    return fa.spv_chain_length(cut) if cut else contextlib.nullcontext()


def synth(spv, sr, cut):
    with cut_of(cut):
        return fa.spv_synthesize(spv, sr)


def synth_dev(spv, sr, cut):
    """the _dev form with its workspace filled with 0xFF and its output with NaN beforehand"""
    dev = torch.device("cuda", 0)
    ch, n, N, _ = spv.shape
    d_spv = torch.from_numpy(np.ascontiguousarray(spv)).to(dev)
    d_out = torch.full((ch, n), float("nan"), dtype=torch.float32, device=dev)
    with cut_of(cut):
        d_ws = torch.full((fa.spv_synthesize_workspace_bytes(ch, n, N, sr),), 0xFF, dtype=torch.uint8, device=dev)
        fa.spv_synthesize_dev(d_spv, ch, n, N, sr, d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def judge(name, regime, got, want, truth):
    """prints every figure, then returns the list of bounds missed (empty: the case holds)"""
    assert got.shape == want.shape and got.dtype == F32 and np.isfinite(got).all()
    r_rms, r_max = R.synthesis_errors(got, want)
    t_rms, t_max = R.synthesis_errors(got, truth)
    o_rms, o_max = R.synthesis_errors(want, truth)
    print("SPV synthesis %-26s vs restatement rel rms %.3e max/peak %.3e; vs truth %.3e %.3e (the restatement: %.3e %.3e; ratios %.2f %.2f)"
          % (name, r_rms, r_max, t_rms, t_max, o_rms, o_max, t_rms / o_rms, t_max / o_max))
    missed = []
    if not (r_rms <= REST_BOUND[regime][0] and r_max <= REST_BOUND[regime][1]):
        missed.append(("restatement", regime, r_rms, r_max))
    if not (t_rms <= TRUTH_FACTOR * o_rms and t_max <= TRUTH_FACTOR * o_max):
        missed.append(("truth", t_rms, t_max, o_rms, o_max))
    return missed


@pytest.mark.parametrize("name", R.SYN_IDS)
def test_against_the_restatement_and_the_truth(name):
    c = R.syn_case(name)
    want, truth = R.syn_expected(name)
    got = synth(R.spv_case(name), c["sr"], c["cut"])
    assert not judge(name, c["regime"], got, want, truth)


# ---------------------------------------------------------------------------------------------------------------------------------
# the real pipeline: the device analysis of noise, as it is and after the constant forms of modify_frequency / repitch
# ---------------------------------------------------------------------------------------------------------------------------------
VARIANTS = {"as_is": None, "repitch_1.25": (1.25, 1), "repitch_0.8": (0.8, 1), "set_440.5": (440.5, 0)}
_pipeline = {}


def pipeline(N, variant):
    """(spv, restatement, truth) of 2 channels x ( 4 L + 37 ) frames of noise through spv_analyze_dev [-> spv_modify_frequency_const_dev],
    under the library's own cuts; computed once"""
    if (N, variant) not in _pipeline:
        dev = torch.device("cuda", 0)
        ch, n = 2, 8 * N + 37
        x = (0.5 * np.random.default_rng(N).standard_normal((ch, n))).astype(F32)
        d_spv = torch.empty((ch, n, N, 2), dtype=torch.float32, device=dev)
        fa.spv_analyze_dev(torch.from_numpy(x).to(dev), ch, n, SR, N, d_spv)
        if VARIANTS[variant] is not None:
            value, multiply = VARIANTS[variant]
            fa.spv_modify_frequency_const_dev(d_spv, ch, n, N, value, multiply, d_spv)
        torch.cuda.synchronize()
        spv = d_spv.cpu().numpy()
        ph = R.inverse_phases(spv[..., 1], SR)
        _pipeline[(N, variant)] = (spv, R.synthesize_np(spv, SR, ph), R.synthesis_truth(spv, SR, ph))
        for a in _pipeline[(N, variant)]:
            a.setflags(write=False)
    return _pipeline[(N, variant)]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("N", [100, 513])
def test_the_real_pipeline(N, variant):
    spv, want, truth = pipeline(N, variant)
    assert np.isfinite(spv).all()
    if variant == "set_440.5":
        assert np.all(spv[..., 1] == F32(440.5))
    assert not judge("pipeline N=%d %s" % (N, variant), "wide", synth(spv, SR, None), want, truth)


# ---------------------------------------------------------------------------------------------------------------------------------
# properties
# ---------------------------------------------------------------------------------------------------------------------------------

def test_channels_are_independent():
    c, spv = R.syn_case("channels"), R.spv_case("channels")
    joint = synth(spv, c["sr"], c["cut"])
    for k in range(c["ch"]):
        assert same_bits(synth(spv[k:k + 1], c["sr"], c["cut"])[0], joint[k]), k
    assert not same_bits(joint[0], joint[1]) and not same_bits(joint[1], joint[2])


@pytest.mark.parametrize("name", ["bins512", "bins4096", "scan17", "fold_any"])
def test_host_and_device_forms_are_bit_identical(name):
    """K = 2 and K = 16; 17 chains through the scan; a rewalked chain"""
    c, spv = R.syn_case(name), R.spv_case(name)
    assert same_bits(synth(spv, c["sr"], c["cut"]), synth_dev(spv, c["sr"], c["cut"]))


CUTS = (1, 32, 97, 4099, None)


@pytest.mark.parametrize("which", ["negative", "wander", "pipeline513"])
def test_the_cut_changes_nothing_beyond_rounding(which):
    """Bit identity is not asked: a carry is the last carry plus a chain's sum, which rounds differently from the sequential sum."""
    if which != "pipeline513":
        spv, (want, truth), regime = R.spv_case(which), R.syn_expected(which), R.syn_case(which)["regime"]
    else:
        (spv, want, truth), regime = pipeline(513, "as_is"), "wide"
    outs = [synth(spv, SR, cut) for cut in CUTS]
    missed = []
    for cut, out in zip(CUTS, outs):
        missed += [(cut,) + m for m in judge("%s cut %s" % (which, cut), regime, out, want, truth) if m[0] == "truth"]
    for i in range(len(CUTS)):
        for j in range(i + 1, len(CUTS)):
            rms, mx = R.synthesis_errors(outs[i], outs[j])
            print("SPV synthesis %s cut %s vs cut %s: rel rms %.3e max/peak %.3e" % (which, CUTS[i], CUTS[j], rms, mx))
            if not (rms <= 2.0 * REST_BOUND[regime][0] and mx <= 2.0 * REST_BOUND[regime][1]):
                missed.append((CUTS[i], CUTS[j], rms, mx))
    assert not missed


def _poison_base():
    """300 bins x 300 frames under a forced cut of 64: frame 150 lies in chain 2, chains 3 and 4 take their carries through
    k_spv_chain_sums and k_spv_scan"""
    c, spv = R.syn_case("wide"), R.spv_case("wide")
    assert (c["n"], c["cut"]) == (300, 64)
    return spv, synth(spv, c["sr"], 64)


def test_later_frames_do_not_reach_earlier_output():
    spv, clean = _poison_base()
    other = spv.copy()
    rng = np.random.default_rng(5)
    other[:, 150:, :, 0] = 10.0 ** rng.uniform(-3.0, 0.0, other[:, 150:, :, 0].shape)
    other[:, 150:, :, 1] = rng.uniform(-24000.0, 96000.0, other[:, 150:, :, 1].shape)
    got = synth(other, SR, 64)
    assert same_bits(got[:, :150], clean[:, :150])
    assert np.all(got[:, 150:] != clean[:, 150:])
    want = R.synthesize_np(other, SR)
    assert not judge("frames >= 150 replaced", "wide", got, want, R.synthesis_truth(other, SR))


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_nan_frequency_poisons_what_follows_and_nothing_before(bad):
    """f = NaN stays NaN through the chain sum and every later carry; f = +inf becomes NaN in the fold (fmod( inf ), as in the
    reference) and reaches the later chains through the scan's own walk of that chain.  Data values only."""
    spv, clean = _poison_base()
    poisoned = spv.copy()
    poisoned[0, 150, 3, 1] = bad
    got = synth(poisoned, SR, 64)
    assert same_bits(got[:, :150], clean[:, :150])
    assert np.isnan(got[:, 150:]).all()
    want = R.synthesize_np(poisoned, SR)
    assert np.array_equal(np.isnan(want), np.isnan(got))
