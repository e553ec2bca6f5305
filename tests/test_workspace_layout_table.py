"""flanhip_synthesize_workspace_bytes over every kernel family, against a recorded table.

The byte count is the last field of the workspace layout, so it moves when any part of the layout does: the chain cut, the groups,
the fix-up words, a family's scratch.  tests/golden/workspace_layout_table.json holds what the library answered, without a device
(cu_count() = 256), before the conversion dispatch was gathered into one route per shape; the layout is part of the ABI (callers size
their workspaces with it), so the answers stay.  Recorded with
    FLAN_AMD_LIB=<a build of the commit to record from>/flan_amd/libflanhip.so python tests/test_workspace_layout_table.py --record
"""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_layout_table.json")
SR = 48000.0

# (window, hop, dft): what serves it
SHAPES = [
    (4096, 256, 8192), (2048, 128, 8192), (8192, 512, 16384), (16384, 4096, 16384),     # team, on the grid
    (4000, 250, 8192), (8000, 500, 16384),                                              # off it: generic dft 8192, mixed-radix dft 16384
    (512, 128, 512), (256, 64, 256), (128, 16, 128),                                    # sub, on the grid
    (500, 125, 512), (512, 384, 512), (256, 50, 256), (100, 25, 128),                   # off it: dft 512 LDS ring, generic
    (2048, 512, 2048), (2048, 128, 2048), (2000, 500, 2048),                            # dft 2048: register accumulator, LDS ring
    (2048, 128, 4096), (2048, 1024, 4096), (2000, 500, 4096),                           # dft 4096: register accumulator, LDS ring
    (4096, 512, 4096), (4000, 1000, 4096),                                              # dft 4096, windows above 2048 (WBIG): both kinds
    (1024, 256, 1024), (1000, 250, 1024),                                               # dft 1024: both kinds
    (64, 16, 64), (32, 8, 32),                                                          # generic
    (3000, 750, 3000), (2048, 512, 6000), (7000, 1750, 16384),                          # mixed-radix; the last with its ring in the workspace
    (2018, 504, 2018), (2048, 512, 2998), (2048, 512, 9998),                            # chirp-z; the last with its buffers in the workspace (glob)
    (4096, 1024, 32768), (32768, 8192, 32768), (2048, 512, 24000),                      # residue-pair: ring in LDS, ring in the workspace, mixed
    (38, 10, 38), (6, 2, 6), (2048, 512, 20006),                                        # direct sums
]
# (channels, frames): 5626 frames = a minute at hop 512; with 256 compute units its 1, 2, 8 and 24 channels lie on both sides of 128 chains
# and of 40 groups per channel at the tuned sizes
CUTS = [(1, 5626), (2, 5626), (8, 5626), (24, 5626), (1024, 40), (1, 40), (2, 300), (8, 100000), (1, 1), (24, 22501)]
HOOKS = [("force_generic", 1), ("no_sub", 1), ("force_direct", 1), ("syn4096_old", 1), ("target_chains", 96)]
HOOK_SHAPES = [(512, 128, 512), (500, 125, 512), (128, 16, 128), (2048, 512, 2048), (2048, 128, 4096), (2000, 500, 4096), (1024, 256, 1024),
               (4096, 256, 8192), (3000, 750, 3000), (2018, 504, 2018), (4096, 1024, 32768)]


def rows():
    """[hook, value, window, hop, dft, channels, frames]: every shape at three cuts (all ten at the sizes with group totals), the hooks at one"""
    out = []
    for i, (w, h, d) in enumerate(SHAPES):
        cuts = CUTS if d in (512, 2048, 4096) and (w, h, d) in HOOK_SHAPES else [CUTS[(i + k * 3) % len(CUTS)] for k in range(3)]
        out += [["", 0, w, h, d, ch, f] for ch, f in cuts]
    for name, value in HOOKS:
        out += [[name, value, w, h, d] + [[1, 5626], [8, 5626]][i % 2] for i, (w, h, d) in enumerate(HOOK_SHAPES)]
    return out


def answer(fa, row):
    name, value, w, h, d, ch, f = row
    ar = float(np.float32(SR) / np.float32(h))
    if not name:
        return fa.synthesize_workspace_bytes(ch, f, d // 2 + 1, SR, ar, w)
    with fa.debug_options(**{name: value}):                      # (cleared in its __exit__, i.e. in a finally)
        return fa.synthesize_workspace_bytes(ch, f, d // 2 + 1, SR, ar, w)


def test_workspace_bytes_match_the_recorded_table():
    import flan_amd as fa
    if fa.lib.flanhip_device_count() != 0:
        pytest.skip("the table is recorded without a device (256 compute units assumed)")
    with open(GOLDEN) as fh:
        table = json.load(fh)
    assert [r[:-1] for r in table] == rows(), "the recorded table is not of these rows: record it again from the commit it was taken on"
    assert 100 <= len(table) <= 260
    wrong = [(r[:-1], r[-1], got) for r in table for got in [answer(fa, r[:-1])] if got != r[-1]]
    assert not wrong, "%d of %d layouts moved, e.g. %s" % (len(wrong), len(table), wrong[:5])
    assert all(r[-1] > 0 for r in table)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import flan_amd as fa
    assert "--record" in sys.argv and fa.lib.flanhip_device_count() == 0
    table = [r + [answer(fa, r)] for r in rows()]
    with open(GOLDEN, "w") as fh:
        fh.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print(len(table), "rows from", fa.LIB_PATH)
