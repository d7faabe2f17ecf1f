"""Dump dm_conv2d_wgrad_plan over a grid that crosses every threshold of the weight-gradient launcher (csrc/backward.hip:
wgrad_route), at the 256-CU count the library assumes without a device: tests/golden/wgrad_plan_256cu.npz, which
tests/test_wgrad_plan_cpu.py replays row for row.

    python tools/wgrad_plan_table.py [--out FILE]           # regenerate from the current library
    python tools/wgrad_plan_table.py --check [FILE]         # compare the current library with a table, print the first differences

Arrays: ``args`` int64 [N, 13] = dy_batch_stride, Cout, x_batch_stride, Cs, NB, H, W, ksize, has_bias, mode,
scratch_floats, io_aligned8, scratch_aligned16 (dm_conv2d_wgrad_plan's, in its order); ``rc`` int32 [N] the return code
(launches, or the negative error); ``rec`` int32 [N, 2 * DM_WGRAD_PLAN_INTS] the records, -1 where nothing is written.
A routing change is meant to show up here: regenerate, and read the diff of the table before committing it."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamask_amd import _abi, _lib  # noqa: E402

DEFAULT = os.path.join(ROOT, 'tests', 'golden', 'wgrad_plan_256cu.npz')
CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_WGRAD_PLAN_INTS'], CONSTS['DM_WGRAD_PLAN_MAX_LAUNCHES']
ATOMICS, SLAB, FX = range(3)
BIG = 1 << 40

COUTS = [1, 5, 16, 32, 33, 36, 37, 64, 65, 128, 200, 256, 1024, 1152]
# J = Cs k^2 on both sides of each TN switch.  64-cout tiles: cost 1.125 x 256 ceil(J / 256) against 1.25 x 128 ceil(J / 128)
# against 1.5 x 64 ceil(J / 64); 128-cout tiles: the last two.  Then the large ones: 2304, and 1024 (3x3 with 1024 couts: 8 x 72
# tiles, more than the 512 a launch is split down to)
CS = {1: [1, 30, 64, 65, 128, 129, 192, 193, 256, 257, 384, 385, 512, 1024, 2304],
      3: [1, 4, 7, 8, 14, 15, 21, 22, 24, 28, 29, 42, 43, 64, 128, 256, 1024, 2304]}
# odd, even, W < 8, one row band / several (28 x 28: 4 bands of 7 rows, 64 x 64: 22 of 3, 40 x 150: one row each), a row that
# does not fit the narrow kernel's 78 KB at all (W = 156; 150: with 32 rows of dy, not with 36)
MAPS = [(7, 7), (14, 14), (6, 6), (1, 8), (28, 28), (64, 64), (40, 150), (2, 156), (3, 9)]
BATCHES = [1, 3, 64, 300]


def plan_of(L):
    def plan(a):
        rec = (ctypes.c_int * (N_INTS * N_REC))(*([-1] * (N_INTS * N_REC)))
        rc = L.dm_conv2d_wgrad_plan(*[int(v) for v in a], rec, N_REC)
        return rc, list(rec)
    return plan


def need(plan, a):
    """Scratch floats the slab route of call ``a`` uses (slabs x stride + splits x bias rows), asked with room for anything."""
    rc, rec = plan(a[:9] + (SLAB, BIG, a[11], 1))
    return rec[13] * rec[16] + rec[11] * rec[15] if rc == 2 else 0


def rows(plan, bound):
    out = []
    for k in (1, 3):
        for cout in COUTS:
            for cs in CS[k]:
                for H, W in MAPS:
                    for nb in BATCHES:
                        if (cout > 256 or cs > 512) and (nb not in (1, 3, 300) or (H, W) not in ((7, 7), (14, 14), (1, 8))):
                            continue
                        a = (cout * H * W, cout, cs * H * W, cs, nb, H, W, k)
                        out.append(a + (0, ATOMICS, 0, 1, 1))
                        out.append(a + (1, FX, 0, 1, 1))
                        out.append(a + (1, SLAB, bound, 1, 1))
                        out.append(a + (1, SLAB, bound, 1, 0))                  # misaligned scratch
                        n = need(plan, a + (1, SLAB, BIG, 1, 1))
                        out.append(a + (1, SLAB, n - 1, 1, 1))                  # one float less than it needs
                        if nb == 3:
                            out.append(a + (1, SLAB, n, 1, 1))                  # ... and exactly that
                            out.append(a + (0, SLAB, bound, 1, 1))
                        if k == 3 and cout <= 36:
                            # what keeps a call off the narrow kernel: misaligned dy / x, odd batch strides
                            out.append(a + (1, SLAB, bound, 0, 1))
                            out.append(a + (1, FX, 0, 0, 1))
                            out.append((a[0] + 1,) + a[1:] + (1, SLAB, bound, 1, 1))
                            out.append(a[:2] + (a[2] + 1,) + a[3:] + (0, ATOMICS, 0, 1, 1))
                            out.append((a[0] + 2, a[1], a[2] + 2) + a[3:] + (1, SLAB, bound, 1, 1))
    # refused calls: every invalid-argument case of the launcher, in each mode
    for mode, ws in ((ATOMICS, 0), (SLAB, bound), (FX, 0), (SLAB, 0), (SLAB, -1)):
        for k in (1, 3, 0, 2, 5, -1):
            for cout, cs, nb, H, W in ((64, 64, 4, 14, 14), (0, 64, 4, 14, 14), (-1, 64, 4, 14, 14), (64, 0, 4, 14, 14), (64, 64, 0, 14, 14),
                                       (64, 64, -1, 14, 14), (64, 64, 4, 0, 14), (64, 64, 4, 14, 0), (64, 64, 4, -14, 14),
                                       (16, 32, 1 << 20, 64, 32), (16, 32, 32768, 256, 256), (16, 32, (1 << 20) - 1, 64, 32),
                                       (16, 32, 1, 1, 0x7fffffff), (16, 32, 2, 1, 0x40000000)):
                for bias in (0, 1):
                    out.append((cout * H * W, cout, cs * H * W, cs, nb, H, W, k, bias, mode, ws, 1, 1))
    return out


def table(L):
    plan = plan_of(L)
    args = np.array(rows(plan, int(L.dm_conv2d_wgrad_scratch_floats())), dtype=np.int64)
    got = [plan(tuple(a)) for a in args.tolist()]
    return args, np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=DEFAULT)
    ap.add_argument('--check', nargs='?', const=DEFAULT)
    o = ap.parse_args()
    L = _lib.lib()
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    if cus != 256 or os.environ.get('DM_WGRAD_WGS'):
        sys.exit(f'the table is the 256-CU one: run without a device, or on one with 256 compute units (this one: {cus}), DM_WGRAD_WGS unset')
    if o.check:
        t = np.load(o.check)
        plan, bad = plan_of(L), 0
        for a, rc, rec in zip(t['args'].tolist(), t['rc'].tolist(), t['rec'].tolist()):
            got = plan(a)
            if got != (rc, rec):
                bad += 1
                if bad <= 10:
                    print('args', a, '\n  table  ', rc, rec, '\n  library', *got)
        print(f'{len(t["rc"])} rows, {bad} differ')
        sys.exit(1 if bad else 0)
    args, rc, rec = table(L)
    np.savez_compressed(o.out, args=args, rc=rc, rec=rec)
    print(f'{o.out}: {len(rc)} rows, {os.path.getsize(o.out)} bytes; return codes', dict(zip(*np.unique(rc, return_counts=True))))


if __name__ == '__main__':
    main()
