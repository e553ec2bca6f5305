"""Audio::mix with grains cut in flight on the MI355X (flan_amd/csrc/grains.hip) against the NumPy restatement (tests/grains_reference.py).

  without the Hann flag   every output bit equals the restatement's ordered fp32 sum; the fused table equals the general path (every grain cut
                          into a buffer of its own first, then mixed through the same kernel) bit for bit; so does the host form
  with it                 | out - truth | <= 4 x max | restatement - truth | per case, the right side computed here on the same input and
                          printed: the device's double cos may differ from libm's in its last places, under a sum whose own rounding dominates
Outputs and workspaces are pre-filled with NaN / 0xFF.  The cases are sized by the kernel's own tile and batch (flanhip_grains_tile_frames,
flanhip_grains_batch_events)."""
import numpy as np
import pytest
import torch

import flan_amd as fa
import grains_reference as R

pytestmark = pytest.mark.gpu
F32 = np.float32
SR = 48000.0
DEV = torch.device("cuda", 0)
T, B = fa.grains_tile_frames(), fa.grains_batch_events()
A_FRAMES, B_FRAMES = 6 * T + 11, 3 * T                       # source A: stereo; source B: mono, behind it
A_OFF, B_OFF = 0, 2 * A_FRAMES


@pytest.fixture(scope="module", autouse=True)
def device():
    assert fa.lib.flanhip_device_count() > 0
    fa.check(fa.lib.flanhip_set_device(0))


def _sources():
    rng = np.random.default_rng(2024)
    n = 2 * A_FRAMES + B_FRAMES
    mag = np.exp2(rng.choice([-20, -10, 0, 10, 20], n)).astype(F32)      # values 2^20 and more apart: a wrong sum order shows
    s = (rng.uniform(-1, 1, n).astype(F32) * mag).astype(F32)
    s[5] = -0.0
    return s


SOURCES = _sources()
GAINS = np.random.default_rng(77).uniform(-2, 2, 40 * T).astype(F32)


def table(rows):
    """rows of ( source 'A' / 'B', s, n, o, sf, ef, gain (a float) or gain offset (an int), flags )"""
    e = R.make_events(len(rows))
    for k, (which, s, n, o, sf, ef, gain, flags) in enumerate(rows):
        stereo = which == "A"
        e["src"][k], e["ch_stride"][k], e["src_frames"][k] = (A_OFF, A_FRAMES, A_FRAMES) if stereo else (B_OFF, B_FRAMES, B_FRAMES)
        e["channels"][k] = 2 if stereo else 1
        e["s"][k], e["n"][k], e["o"][k], e["sf"][k], e["ef"][k], e["flags"][k] = s, n, o, sf, ef, flags
        if isinstance(gain, int):
            e["gain_offset"][k] = gain
        else:
            e["gain"][k] = gain
    return e


def geometry_rows(flags=0):
    return [
        ("A", 3, 3 * T + 5, T // 2, 100, 200, 0.75, flags),                     # spans four tiles
        ("B", 0, 100, T, 10, 10, 1.0, flags),                                   # starts on a tile's first frame; a mono source: channel 1 does not hear it
        ("A", 7, 0, 2 * T, 0, 0, 1.0, flags),                                   # an empty event between live ones
        ("A", 50, T - 37, T + 37, 0, 0, 100, flags),                            # ends on a tile's last frame; per-frame gains
        ("B", 17, 300, -120, 150, 150, -0.5, flags),                            # a negative o; fades that meet
        ("A", 0, 0, 9 * T, 0, 0, 1.0, flags),                                   # an empty event: it alone would make the output longer ...
        ("A", 5, 700, 4 * T - 20, 0, 699, 3 * T + 1, flags),                    # reaches the output's last frame; unsorted start frames from here on
        ("B", 1000, 1, 2 * T - 1, 0, 0, 2.0, flags),                            # n = 1 on a tile's last frame
        ("A", 4, 2, 0, 1, 1, 1.0, flags),                                       # n = 2, fades that meet: both terms are 0
        ("A", 5, 1, 5 * T, 0, 0, 1.0, flags),                                   # a lone -0.0f on channel 0: comes out +0
    ]


def deep_rows(flags=0):
    """more overlapping events on one tile than one LDS batch holds, plus a ragged remainder, in no order of o; every third a mono source"""
    rng = np.random.default_rng(31)
    rows = []
    for k in range(B + 37):
        n = int(rng.integers(40, 2 * T))
        o = int(rng.integers(T - n + 1, 2 * T - 1))                             # every one touches tile 1
        which = "B" if k % 3 == 0 else "A"
        s = int(rng.integers(0, (B_FRAMES if which == "B" else A_FRAMES) - n))
        sf = int(rng.integers(0, n // 2))
        gain = int(rng.integers(0, GAINS.size - n)) if k % 4 == 1 else float(F32(rng.uniform(-1, 1)))
        rows.append((which, s, n, o, sf, n // 2 - sf // 2, gain, flags))
    return rows


def cloud_rows(flags=0, count=3000, frames=90000, seed=5):
    """a granulated texture: sorted starts, grains 10 to 60 ms, ~60 deep"""
    rng = np.random.default_rng(seed)
    rows = []
    for o in np.sort(rng.integers(-1000, frames, count)):
        n = int(rng.integers(480, 2880))
        fade = int(rng.integers(0, n // 2 + 1))
        rows.append(("A", int(rng.integers(0, A_FRAMES - n)), n, int(o), fade, fade, float(F32(rng.uniform(0.1, 1))), flags))
    return rows


PLAIN = {"geometry": geometry_rows, "deep": deep_rows, "cloud": cloud_rows}
HANN = {"geometry": lambda: geometry_rows(R.HANN), "deep": lambda: deep_rows(R.HANN), "cloud": lambda: cloud_rows(R.HANN, 1500, 50000, 6),
        "psola": lambda: [("A", 200 + 3 * k, 436, 218 * k, 0, 0, 1.0, R.HANN) for k in range(200)]}      # 2 periods long, a period apart, no fades left


def dev_mix(ev, sources=SOURCES, gains=GAINS, channels=2, frames=0):
    frames, first, last = fa.grains_plan(ev, frames)
    d_src, d_gains = torch.from_numpy(sources).to(DEV), torch.from_numpy(gains).to(DEV)
    d_out = torch.full((channels, frames), float("nan"), dtype=torch.float32, device=DEV)
    d_ws = torch.full((fa.grains_workspace_bytes(len(ev), frames),), 0xFF, dtype=torch.uint8, device=DEV)
    fa.grains_mix_dev(ev, first, last, d_gains, gains.size, d_src, sources.size, channels, frames, SR, d_out, d_ws)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


_WANT = {}


def want(name):
    """the restatement of a case, computed once"""
    if name not in _WANT:
        ev = table(PLAIN[name]())
        _WANT[name] = (ev, R.mix32(ev, SOURCES, GAINS, 2, R.out_frames(ev), SR))
    return _WANT[name]


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_the_mix_is_the_restatement_s_bit_for_bit(name):
    ev, expected = want(name)
    got = dev_mix(ev)
    assert got.shape == expected.shape and not np.isnan(got).any()
    assert R.same_bits(got, expected), np.argwhere(got.view(np.uint32) != expected.view(np.uint32))[:5]


def test_the_geometry_case_is_what_it_says():
    ev, expected = want("geometry")
    frames, first, last = fa.grains_plan(ev)
    assert frames == 9 * T and frames == R.out_frames(ev)                       # the empty event at 9 T sets the length
    ev2 = ev.copy()
    ev2["o"][5] = 0
    assert fa.grains_plan(ev2)[0] == 5 * T + 1                                  # without it: not a multiple of the tile
    got = dev_mix(ev2)
    assert R.same_bits(got, expected[:, :5 * T + 1])
    assert np.all(expected[:, 5 * T + 1:] == 0)
    assert not np.signbit(got[0, 5 * T]) and got[0, 5 * T] == 0 and np.signbit(SOURCES[5])       # the lone -0.0f
    # a wrong order of additions would show: the reversed table gives other bits
    order = list(range(len(ev)))[::-1]
    assert not R.same_bits(R.mix32(ev, SOURCES, GAINS, 2, frames, SR, order=order), expected)
    deep, deep_expected = want("deep")
    assert np.any(np.diff(deep["o"]) < 0)
    assert not R.same_bits(R.mix32(deep, SOURCES, GAINS, 2, deep_expected.shape[1], SR, order=list(range(len(deep)))[::-1]), deep_expected)
    first, last = fa.grains_plan(deep)[1:]
    assert last[1] - first[1] + 1 == B + 37                                     # one full batch and a ragged one on tile 1


def test_an_output_shorter_than_the_events_clips_them():
    ev, expected = want("deep")
    frames = T + T // 2 + 3
    assert R.same_bits(dev_mix(ev, frames=frames), expected[:, :frames])


def test_zero_events_give_positive_zeros():
    got = dev_mix(R.make_events(0), frames=T + 5)
    assert got.shape == (2, T + 5) and np.all(got == 0) and not np.signbit(got).any()
    ev = table([("A", 0, 0, 3, 0, 0, 1.0, 0), ("B", 0, 0, 2 * T + 1, 0, 0, 1.0, 0)])      # only empty events
    got = dev_mix(ev)
    assert got.shape == (2, 2 * T + 1) and np.all(got == 0) and not np.signbit(got).any()


def test_mono_output_and_more_channels_than_any_source():
    ev, _ = want("geometry")
    mono = dev_mix(ev, channels=1)
    assert R.same_bits(mono, R.mix32(ev, SOURCES, GAINS, 1, mono.shape[1], SR))
    three = dev_mix(ev, channels=3)
    assert R.same_bits(three[:2], want("geometry")[1]) and np.all(three[2] == 0)


@pytest.mark.parametrize("name", sorted(PLAIN))
def test_the_fused_path_equals_the_general_path(name):
    """the general path: every grain cut, faded and written to a buffer of its own, then mixed as a plain event with its gain"""
    ev, expected = want(name)
    plain_ev, grains = R.materialise(ev, SOURCES, GAINS, SR)
    assert np.all(plain_ev["sf"] == 0) and np.all(plain_ev["flags"] == 0)
    got = dev_mix(plain_ev, sources=grains)
    assert R.same_bits(got, expected)


def test_the_host_form_and_device_addresses():
    ev, expected = want("geometry")
    assert R.same_bits(fa.grains_mix(ev, GAINS, SOURCES, 2, expected.shape[1], SR), expected)
    # sources named by their device addresses, no base
    d_src, d_gains = torch.from_numpy(SOURCES).to(DEV), torch.from_numpy(GAINS).to(DEV)
    absolute = ev.copy()
    absolute["src"] = np.uint64(d_src.data_ptr()) + np.uint64(4) * ev["src"]
    frames, first, last = fa.grains_plan(absolute)
    d_out = torch.full((2, frames), float("nan"), dtype=torch.float32, device=DEV)
    d_ws = torch.full((fa.grains_workspace_bytes(len(ev), frames),), 0xFF, dtype=torch.uint8, device=DEV)
    fa.grains_mix_dev(absolute, first, last, d_gains, GAINS.size, None, 0, 2, frames, SR, d_out, d_ws)
    torch.cuda.synchronize()
    assert R.same_bits(d_out.cpu().numpy(), expected)


@pytest.mark.parametrize("name", sorted(HANN))
def test_hann_grains_stay_within_four_times_the_restatement_s_error(name):
    ev = table(HANN[name]())
    frames = R.out_frames(ev)
    truth = R.mix64(ev, SOURCES, GAINS, 2, frames, SR)
    restated = R.mix32(ev, SOURCES, GAINS, 2, frames, SR)
    got = dev_mix(ev)
    assert got.shape == truth.shape and not np.isnan(got).any()
    bound = np.abs(restated.astype(np.float64) - truth).max()
    error = np.abs(got.astype(np.float64) - truth).max()
    differing = np.count_nonzero(got.view(np.uint32) != restated.view(np.uint32))
    print("hann %-8s | restatement - truth | %.6g   | device - truth | %.6g   ratio %.4f   samples that differ from the restatement %d of %d"
          % (name, bound, error, error / bound if bound else 0.0, differing, got.size))
    assert bound > 0
    assert error <= 4 * bound
