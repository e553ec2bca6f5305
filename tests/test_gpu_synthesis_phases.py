"""The phased walk of k_synthesize_v2 (pv_kernels_v2.h): a chain that settles its overlaps inside the kernel, is not a channel's chain 0 and has a head of
whole frames stores its head frames in a loop of their own (agent-scope stores into the head buffer) and the frames behind them in another (plain stores into
the output); everything else (hop 128 included: its phase loops ran short of registers) walks the general loop.  Same operations in the same order on every sample, so the fused round trip must give THE SAME BITS as
the same call with the overlaps added by the separate launch (k_ola_fixup4, FLANHIP_DEBUG_INLINE_FIXUP = 2, which walks the general loop) -- and the
synthesis must agree with the oracle's on the same PV within P2 of tests/test_gpu_conversions.py (RMS of the difference <= 1e-5 of unit scale).

Shapes: dft 2048, 48 kHz, 2 channels x 1.5 s and 1 channel x 0.3 s (chain 0, the last chain and a channel of one group are most of the work there).  Chain
lengths are forced (FLANHIP_DEBUG_CHAIN_LEN) around i_pub + 3, the shortest chain that takes the phased walk: i_pub = ceil( ( window - hop ) / hop ) is the
frame that publishes the head.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SR = 48000.0
DFT = 2048
P2_RMS = 1e-5                  # tests/test_gpu_conversions.py, test_synthesis_parity: the same bound, not a wider one
SIZES = {"2ch_1.5s": (2, 72000), "1ch_0.3s": (1, 14400)}


def i_pub(window, hop):
    return -(-(window - hop) // hop)


def _cases():
    out = []
    for hop in (1024, 512, 256, 128):                            # 1, 3, 7 and 15 head frames
        for extra in (3, 4, 7, 2):                               # the shortest phased chain, one and four body frames more; 2: k_ola_fixup4's route
            out.append((2048, hop, i_pub(2048, hop) + extra))
    for extra in (3, 7):
        out.append((1024, 256, i_pub(1024, 256) + extra))        # the head is whole frames and the window shorter than the transform
        out.append((1920, 512, i_pub(1920, 512) + extra))        # a head of 2.75 hops: the general walk
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def fa():
    import flan_amd
    assert flan_amd.lib.flanhip_device_count() > 0
    return flan_amd


@pytest.fixture(scope="module")
def signals():
    """per size: the input on the device (made once, never written again)"""
    import torch
    import flan_amd as fa
    dev = torch.device("cuda", 0)
    sig = {}
    for name, (ch, n) in SIZES.items():
        x = torch.empty((ch, n), dtype=torch.float32, device=dev)
        fa.check(fa.lib.flanhip_noise_dev(ctypes.c_void_p(x.data_ptr()), ch, n, 2024, None))
        sig[name] = x
    torch.cuda.synchronize()
    return sig


_ORACLE = {}


def oracle_audio(key, pv_host, ar, window):
    """the oracle's synthesis of this PV: once per ( size, window, hop ) -- the PV does not depend on the chain length (the fused analysis is held
    bit-identical across chain lengths by tests/test_gpu_conversions.py), which the caller checks against the kept copy"""
    if key not in _ORACLE:
        ref, flag = O.synthesize(pv_host, SR, ar, window)
        assert flag == 0
        _ORACLE[key] = (pv_host.copy(), ref.astype(np.float64))
    kept_pv, ref = _ORACLE[key]
    assert np.array_equal(kept_pv.view(np.uint32), pv_host.view(np.uint32))
    return ref


def round_trip(fa, x, window, hop, chain_len, inline_fixup):
    import torch
    ch, n = x.shape
    bins = DFT // 2 + 1
    F = int(fa.lib.flanhip_num_pv_frames(n, hop))
    ar = SR / hop
    with fa.debug_options(chain_len=chain_len, inline_fixup=inline_fixup):
        pv = torch.empty((ch, F, bins, 2), dtype=torch.float32, device=x.device)
        out = torch.full((ch, F * hop), float("nan"), dtype=torch.float32, device=x.device)
        ws = torch.empty(fa.synthesize_workspace_bytes(ch, F, bins, SR, ar, window), dtype=torch.uint8, device=x.device)
        flag = torch.zeros(1, dtype=torch.int32, device=x.device)
        fa.analyze_dev_fused(x, ch, n, SR, window, hop, DFT, pv, ws, None)
        fa.synthesize_dev_fused(pv, ch, F, bins, SR, ar, window, out, ws, flag, None)
        torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return pv, out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("window,hop,chain_len", CASES, ids=["w%d_hop%d_L%d" % c for c in CASES])
def test_phased_walk_equals_the_separate_fixup_and_the_oracle(fa, signals, size, window, hop, chain_len):
    import torch
    x = signals[size]
    pv, out = round_trip(fa, x, window, hop, chain_len, 0)              # the library's choice: inside the kernel from i_pub + 3 frames per chain on
    pv2, want = round_trip(fa, x, window, hop, chain_len, 2)            # the overlaps by k_ola_fixup4
    assert torch.equal(pv.view(torch.int32), pv2.view(torch.int32))
    diff = out.view(torch.int32) != want.view(torch.int32)
    ndiff = int(diff.sum().item())
    first = diff.nonzero()[0].tolist() if ndiff else None
    print("\n[phases %s w%d hop%d L%d] %d of %d samples differ from the separate launch's%s" % (size, window, hop, chain_len, ndiff, out.numel(),
                                                                                               "" if not ndiff else ", first at %s" % first))
    assert ndiff == 0
    ref = oracle_audio((size, window, hop), pv.cpu().numpy(), np.float32(SR) / np.float32(hop), window)
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape
    rms = float(np.sqrt(np.mean((got - ref) ** 2)))
    print("[phases %s w%d hop%d L%d] synthesis against the oracle on the same PV: rms diff=%.3e" % (size, window, hop, chain_len, rms))
    assert rms <= P2_RMS


def test_phased_walk_on_two_streams_gives_the_same_bits_every_launch(fa, signals):
    """The head's publication now sits at the top of the second phase: 30 fused round trips on each of two streams at once (a workspace each), every one
    of the 60 outputs compared bit for bit with the separate-launch form.  A soak of correct code."""
    import torch
    x = signals["2ch_1.5s"]
    ch, n = x.shape
    window, hop = 2048, 512
    chain_len = i_pub(window, hop) + 4
    bins = DFT // 2 + 1
    F = int(fa.lib.flanhip_num_pv_frames(n, hop))
    ar = SR / hop
    _, want = round_trip(fa, x, window, hop, chain_len, 2)
    streams = [torch.cuda.Stream(device=x.device) for _ in range(2)]
    bad = checked = 0
    with fa.debug_options(chain_len=chain_len):
        bufs = [(torch.empty((ch, F, bins, 2), dtype=torch.float32, device=x.device), torch.empty((ch, F * hop), dtype=torch.float32, device=x.device),
                 torch.empty(fa.synthesize_workspace_bytes(ch, F, bins, SR, ar, window), dtype=torch.uint8, device=x.device)) for _ in streams]
        try:
            for _ in range(30):
                for (pv, out, ws), s in zip(bufs, streams):
                    out.fill_(float("nan"))
                for (pv, out, ws), s in zip(bufs, streams):
                    st = int(s.cuda_stream)
                    s.wait_stream(torch.cuda.current_stream())
                    fa.analyze_dev_fused(x, ch, n, SR, window, hop, DFT, pv, ws, st)
                    fa.synthesize_dev_fused(pv, ch, F, bins, SR, ar, window, out, ws, None, st)
                torch.cuda.synchronize()
                for pv, out, ws in bufs:
                    checked += 1
                    bad += 0 if torch.equal(out.view(torch.int32), want.view(torch.int32)) else 1
        finally:
            torch.cuda.synchronize()
    print("\n[phases two streams] %d outputs compared, %d differing" % (checked, bad))
    assert checked == 60 and bad == 0
