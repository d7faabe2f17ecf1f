"""Dump dm_deform_conv_plan over a grid that crosses every threshold of the DCN forward launcher, at the 256-CU count the
library assumes without a device: tests/golden/dcn_plan_256cu.npz, which tests/test_dcn_plan_cpu.py replays row for row.

    python tools/dcn_plan_table.py [--out FILE]           # regenerate from the current library
    python tools/dcn_plan_table.py --check [FILE]         # compare the current library with a table, print the first differences

Arrays: ``args`` int64 [N, 9] = NB, C, H, W, Cout, deform_groups, flags, workspace_floats, M2; ``rc`` int32 [N] the return
code (launches, or the negative error); ``rec`` int32 [N, 2 * DM_DCN_PLAN_INTS] the records, -1 where nothing is written.
A routing change is meant to show up here: regenerate, and read the diff of the table before committing it."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamask_amd import _abi, _lib  # noqa: E402

DEFAULT = os.path.join(ROOT, 'tests', 'golden', 'dcn_plan_256cu.npz')
CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_DCN_PLAN_INTS'], CONSTS['DM_DCN_PLAN_MAX_LAUNCHES']

BATCHES = [1, 2, 3, 8, 16, 24, 25, 37, 38, 39, 47, 48, 49, 64, 75, 76, 77, 100, 128, 129, 150, 151, 152, 167, 168, 169, 196, 197,
           256, 512, 520, 1000]
MAPS = [(14, 14), (16, 16), (11, 12), (15, 15), (10, 10), (7, 7), (16, 28), (16, 32), (16, 36), (28, 28), (56, 56), (20, 60),
        (16, 24), (64, 64)]
COUTS = [16, 32, 33, 64, 65, 128, 129, 224, 225, 250, 256]
BIG = 1 << 40


def plan(L, a):
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([-1] * (N_INTS * N_REC)))
    rc = L.dm_deform_conv_plan(*[int(v) for v in a], rec, N_REC)
    return rc, list(rec)


def rows(L):
    out = []
    for H, W in MAPS:
        for nb in BATCHES:
            for c in (16, 256):
                for cout in COUTS:
                    per = nb * cout * H * W
                    # no workspace; what dm_deform_conv_splitk_floats asks for; one float short of one / of three copies of
                    # the output (no split at all / not the three of the 25 .. 128-RoI rule); more than anything needs
                    for ws in sorted({0, int(L.dm_deform_conv_splitk_floats(nb, c, H, W, cout)), per - 1, 3 * per - 1, BIG}):
                        for flags in (0, 8):
                            out.append((nb, c, H, W, cout, 1, flags, ws, 0))
            # the chained 1x1 (Cout == C == 64 / 128 where the band kernel takes the map), with the plain call beside it
            for c, cout in ((64, 64), (128, 128), (256, 64), (64, 128)):
                for m2 in (0, cout // 2 - 2, cout // 2 + 31):
                    out.append((nb, c, H, W, cout, 1, 1, 0, m2))
                out.append((nb, c, H, W, cout, 1, 1, BIG, 0))
    # refused calls, alone and in pairs (the precedence of the checks), plain and chained
    for m2 in (0, 30):
        for H, W in ((14, 14), (16, 28), (28, 28)):
            for nb in (0, 1, 100, -1):
                for c, cout, dg in ((16, 16, 3), (16, 64, 4), (20, 64, 1), (64, 64, 0), (64, 64, 3), (64, 64, 16), (64, 64, 1)):
                    for flags in (0, 1, 8, 16, 17):
                        out.append((nb, c, H, W, cout, dg, flags, 0, m2))
                        if m2 == 0:
                            out.append((nb, c, H, W, cout, dg, flags, BIG, m2))
        for nb in (0, 1, 100):
            for H, W in ((14, 1), (1, 1), (300, 1), (14, 2), (0, 14), (14, 0), (16, 0)):
                for flags in (0, 16):
                    out.append((nb, 64, H, W, 64, 1, flags, 0, m2))
                    out.append((nb, 60, H, W, 64, 1, flags, 0, m2))
        out.append((1 << 20, 64, 64, 32, 64, 1, 0, 0, m2))              # 2^31 pixels
        out.append((32768, 64, 256, 256, 64, 1, 0, 0, m2))
        out.append((100, 64, 28, 28, 0, 1, 0, 0, m2))
        out.append((100, 0, 28, 28, 64, 1, 0, 0, m2))
    return out


def table(L):
    args = np.array(rows(L), dtype=np.int64)
    got = [plan(L, a) for a in args]
    return args, np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=DEFAULT)
    ap.add_argument('--check', nargs='?', const=DEFAULT)
    o = ap.parse_args()
    L = _lib.lib()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    if cus != 256:
        sys.exit(f'the table is the 256-CU one: run without a device, or on one with 256 compute units (this one: {cus})')
    if o.check:
        t = np.load(o.check)
        bad = 0
        for a, rc, rec in zip(t['args'], t['rc'], t['rec']):
            got = plan(L, a)
            if got != (int(rc), [int(v) for v in rec]):
                bad += 1
                if bad <= 10:
                    print('args', list(a), '\n  table  ', int(rc), list(rec), '\n  library', *got)
        print(f'{len(t["rc"])} rows, {bad} differ')
        sys.exit(1 if bad else 0)
    args, rc, rec = table(L)
    np.savez_compressed(o.out, args=args, rc=rc, rec=rec)
    print(f'{o.out}: {len(rc)} rows, {os.path.getsize(o.out)} bytes; return codes', dict(zip(*np.unique(rc, return_counts=True))))


if __name__ == '__main__':
    main()
