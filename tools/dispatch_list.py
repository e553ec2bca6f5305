"""One fused round trip (analyze_dev_fused, synthesize_dev_fused) and one unfused synthesize_dev per shape, over every kernel family of the
PV conversions: run under a kernel trace, the ordered list of kernel names, grids, workgroups and LDS sizes is what the host dispatch of
conversions.hip decides.  Two builds dispatch alike when their lists are equal (FLAN_AMD_LIB selects the library); the printed digests of
the outputs compare what they computed.
    rocprofv3 --kernel-trace --output-format csv -d out -- python tools/dispatch_list.py"""
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import flan_amd as fa

SR = 48000.0
# (window, hop, dft, channels, seconds)
SHAPES = [
    (4096, 256, 8192, 2, 4), (2048, 128, 8192, 1, 3), (8192, 512, 16384, 2, 4), (16384, 4096, 16384, 1, 4),      # team
    (4000, 250, 8192, 2, 3), (8000, 500, 16384, 1, 3),                                                          # off its grid: generic, mixed-radix
    (512, 128, 512, 8, 4), (256, 64, 256, 2, 3), (128, 16, 128, 1, 2), (512, 64, 512, 1, 20),                    # sub (the last with group totals)
    (500, 125, 512, 2, 3), (512, 384, 512, 1, 3), (256, 50, 256, 2, 2), (100, 25, 128, 1, 2),                    # off its grid
    (2048, 512, 2048, 8, 4), (2048, 128, 2048, 2, 3), (2048, 1024, 2048, 1, 3), (2000, 500, 2048, 2, 3),         # dft 2048, both kinds
    (2048, 128, 4096, 2, 4), (2048, 1024, 4096, 1, 3), (2000, 500, 4096, 2, 3), (4096, 512, 4096, 2, 3), (4000, 1000, 4096, 1, 3),
    (1024, 256, 1024, 8, 4), (1024, 128, 1024, 1, 3), (1000, 250, 1024, 2, 3),                                   # dft 1024, both kinds
    (64, 16, 64, 2, 1), (32, 8, 32, 1, 1),                                                                      # generic
    (3000, 750, 3000, 2, 3), (2048, 512, 6000, 1, 3), (7000, 1750, 16384, 1, 3),                                 # mixed-radix
    (2018, 504, 2018, 2, 3), (2048, 512, 2998, 1, 3), (2048, 512, 9998, 1, 2),                                   # chirp-z
    (4096, 1024, 32768, 2, 3), (32768, 8192, 32768, 1, 3), (2048, 512, 24000, 1, 2),                             # residue pairs
    (38, 10, 38, 2, 1), (6, 2, 6, 1, 1),                                                                        # direct sums
    (2048, 512, 2048, 1, 60), (2048, 128, 4096, 1, 60),                                                         # long enough for the group totals
]


def main():
    dev = torch.device("cuda", 0)
    fa.check(fa.lib.flanhip_set_device(0))
    for w, hop, dft, ch, secs in SHAPES:
        n, bins, ar = int(secs * SR), dft // 2 + 1, SR / hop
        F = int(fa.lib.flanhip_num_pv_frames(n, hop))
        audio = torch.empty((ch, n), dtype=torch.float32, device=dev)
        fa.check(fa.lib.flanhip_noise_dev(ctypes.c_void_p(audio.data_ptr()), ch, n, 1, None))
        pv = torch.empty((ch, F, bins, 2), dtype=torch.float32, device=dev)
        out = torch.empty((ch, F * hop), dtype=torch.float32, device=dev)
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.zeros(fa.synthesize_workspace_bytes(ch, F, bins, SR, ar, w), dtype=torch.uint8, device=dev)
        fa.analyze_dev_fused(audio, ch, n, SR, w, hop, dft, pv, ws, None)
        fa.synthesize_dev_fused(pv, ch, F, bins, SR, ar, w, out, ws, flag, None)
        torch.cuda.synchronize()
        fused = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
        fa.synthesize_dev(pv, ch, F, bins, SR, ar, w, out, ws, flag, None)
        torch.cuda.synchronize()
        plain = hashlib.sha1(out.cpu().numpy().tobytes()).hexdigest()[:12]
        print("%5d %5d %6d  %d ch x %2d s  pv %s  out %s / %s  flag %d" % (w, hop, dft, ch, secs, hashlib.sha1(pv.cpu().numpy().tobytes()).hexdigest()[:12],
                                                                          fused, plain, int(flag.item())), flush=True)


if __name__ == "__main__":
    main()
