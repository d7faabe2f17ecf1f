"""Dump dm_bwd_plan over a grid that crosses every threshold of the six training-side launchers of csrc/backward.hip
(im2col_route, coord_grad_route, col2im_route, upsample_bwd_route, point_sample_bwd_route, class_logits_bwd_route), at the
256-CU count the library assumes without a device: tests/golden/bwd_plan_256cu.npz, which tests/test_bwd_plan_cpu.py replays
row for row.

    python tools/bwd_plan_table.py [--out FILE]           # regenerate from the current library
    python tools/bwd_plan_table.py --check [FILE]         # compare the current library with a table, print the first differences

Arrays: ``op`` int32 [N] (DM_BWD_*); ``args`` int64 [N, 7] the op's numbers in dm_bwd_plan's order, zeros after the last;
``rc`` int32 [N] the return code (launches, or the negative error); ``rec`` int32 [N, 2 * DM_BWD_PLAN_INTS] the records, -1
where nothing is written.  A routing change is meant to show up here: regenerate, and read the diff of the table before
committing it."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamask_amd import _abi, _lib  # noqa: E402

DEFAULT = os.path.join(ROOT, 'tests', 'golden', 'bwd_plan_256cu.npz')
CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_BWD_PLAN_INTS'], CONSTS['DM_BWD_PLAN_MAX_LAUNCHES']
IM2COL, COORD_GRAD, COL2IM, UPSAMPLE, POINT_SAMPLE, CLASS_LOGITS = range(6)
COUNTS = (5, 5, 5, 4, 7, 7)
ATOMICS, SLAB, FX = range(3)
BIG = 1 << 40

# --- the three DCN launchers: NB, C, H, W, deform_groups
# channels per deformable group: every CT's divisibility (im2col 32 / 16 / 8 / 4, col2im 8 / 4 / 2 / 1, coordinate gradient 8)
CPG = [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64]
DCN_MAPS = [
    (1, 1), (5, 1), (1, 2), (2, 2), (5, 7), (9, 9), (7, 9), (10, 6), (20, 12), (14, 14), (24, 24), (28, 28), (56, 56),       # H W % 4, W < 2
    # im2col: CT H W 4 bytes on both sides of 64 KB: H W = 512 | 516 (CT 32), 1024 | 1028 (16), 2048 | 2052 (8), 4096 | 4100 (4)
    (16, 32), (12, 43), (32, 32), (4, 257), (32, 64), (36, 57), (64, 64), (50, 82),
    # col2im: CT H W 8 bytes: 1024 | 1025 (CT 8), 2048 | 2052 (4), 4096 | 4097 (2), 8192 | 8194 (1: beyond it the call is refused)
    (25, 41), (17, 241), (64, 128), (2, 4097),
    # coordinate gradient: slots = 2 (XR + 2)(W + 2) at 1024 | 1088 | 1152 (a multi-band map) and 2040 | 2070; W at 224 | 225;
    # 9 BRows W at 2043 | 2052 (W 227 | 228: BRows 1); H W at 2^20 - 32 | 2^20 + 192
    (14, 30), (15, 30), (16, 30), (64, 66), (64, 67), (3, 224), (300, 224), (3, 225), (3, 227), (3, 228), (4681, 224), (4682, 224),
]
DCN_REFUSED = [(-1, 16, 14, 14, 2), (2, 0, 14, 14, 2), (2, -8, 14, 14, 2), (2, 16, 0, 14, 2), (2, 16, -1, 14, 2), (2, 16, 14, 0, 2),
               (2, 16, 14, -2, 2), (2, 16, 14, 14, 0), (2, 16, 14, 14, -1), (2, 6, 14, 14, 4), (2, 16, 14, 14, 3),
               # an invalid argument is decided before W < 2, W < 2 before the empty call; an empty call is never refused
               (2, 0, 14, 1, 2), (-1, 16, 14, 1, 2), (0, 16, 14, 1, 2), (0, 0, 14, 14, 2), (0, 16, 4682, 224, 2), (0, 6, 14, 14, 4)]

# --- upsample: NC, H, W, align_corners.  16 H W at 64 KB and 24 H W at 96 KB: both H W = 4096 | 4098 | 4160; H or W = 1;
# NC at 2 CUs = 512 | 513 and at the 8 CUs = 2048 | 2049 workgroups a launch has at most
UP_MAPS = [(1, 1), (1, 5), (5, 1), (2, 2), (2, 3), (9, 13), (14, 14), (56, 56), (64, 64), (64, 65), (65, 64), (2, 2048), (2, 2049),
           (72, 72), (112, 112)]
UP_NC = [0, 1, 30, 512, 513, 2048, 2049, 5000]
UP_REFUSED = [(-1, 14, 14), (4, 0, 14), (4, 14, 0), (4, -1, 14), (4, 14, -3), (0, 0, 14), (-1, 1, 1)]

# --- point sample: B, C, H, W, N, S, fx.  The gather kernel's LDS: 4 (4 S^2 + 4 S + 3 (W + 4) + 3 (H + 4)) bytes at 64 KB:
# S = 63: H + W = 77 | 78; S = 64 never fits; S at 128 | 129; H W^2 at 2^32: 1000 x 2072 | 2073
PS_MAPS = [(25, 42), (64, 80), (30, 47), (30, 48), (1, 1), (200, 304), (1000, 2072), (1000, 2073)]
PS_S = [1, 7, 14, 28, 56, 62, 63, 64, 112, 127, 128, 129, 200]
PS_REFUSED = [(0, 8, 25, 42, 3, 14), (2, 0, 25, 42, 3, 14), (2, 8, 0, 42, 3, 14), (2, 8, 25, 0, 3, 14), (2, 8, 25, 42, -1, 14),
              (2, 8, 25, 42, 3, 0), (2, 8, 25, 42, 3, -1), (2, 8, 25, 42, 0, 0), (-1, 8, 25, 42, 0, 14)]

# --- class logits: N, C, HW, num_classes, mode, aligned16, scratch_floats.  HW % 4, HW at 256 | 260 and 1024 | 1028
CL_HW = [1, 4, 81, 196, 252, 255, 256, 260, 784, 1024, 1028, 1156]
CL_N = [0, 1, 7, 1100]
CL_C = [1, 16, 17, 40, 64, 256]
CL_NC = [1, 80, 65535, 65536]
CL_REFUSED = [(-1, 64, 196, 80), (7, 0, 196, 80), (7, -4, 196, 80), (7, 64, 0, 80), (7, 64, -4, 80), (7, 64, 196, 0), (7, 64, 196, -1),
              (0, 0, 196, 80), (0, 64, 196, 0)]


def plan_of(L):
    def plan(op, a):
        rec = (ctypes.c_int * (N_INTS * N_REC))(*([-1] * (N_INTS * N_REC)))
        nums = (ctypes.c_longlong * COUNTS[op])(*[int(v) for v in a[:COUNTS[op]]])
        rc = L.dm_bwd_plan(op, nums, COUNTS[op], rec, N_REC)
        return rc, list(rec)
    return plan


def clb_need(n, c):
    return 2 * n * c + 2 * n         # dm_class_logits_bwd_scratch_floats


def rows():
    out = []
    for op in (IM2COL, COORD_GRAD, COL2IM):
        for H, W in DCN_MAPS:
            for cpg in CPG:
                for dg in (1, 2, 4):
                    for nb in (1, 3):
                        out.append((op, nb, cpg * dg, H, W, dg))
            out.append((op, 0, 16, H, W, 2))
        out += [(op,) + a for a in DCN_REFUSED]
    for ac in (0, 1, 2):
        for H, W in UP_MAPS:
            out += [(UPSAMPLE, nc, H, W, ac) for nc in UP_NC]
        out += [(UPSAMPLE,) + a + (ac,) for a in UP_REFUSED]
    for fx in (0, 1):
        for H, W in PS_MAPS:
            for S in PS_S:
                for C in (1, 4, 5, 22, 256):
                    out += [(POINT_SAMPLE, B, C, H, W, N, S, fx) for B, N in ((1, 1), (2, 11), (2, 300), (2, 0))]
        out += [(POINT_SAMPLE,) + a + (fx,) for a in PS_REFUSED]
    for hw in CL_HW:
        for n in CL_N:
            for c in CL_C:
                for nc in CL_NC:
                    for al in (1, 0):
                        out.append((CLASS_LOGITS, n, c, hw, nc, ATOMICS, al, 0))
                        out.append((CLASS_LOGITS, n, c, hw, nc, FX, al, 0))
                        out.append((CLASS_LOGITS, n, c, hw, nc, SLAB, al, clb_need(n, c)))
                    out.append((CLASS_LOGITS, n, c, hw, nc, SLAB, 1, BIG))
                    out.append((CLASS_LOGITS, n, c, hw, nc, SLAB, 1, clb_need(n, c) - 1))         # one float less than it needs
    # refused calls, in each mode; a slab call is refused for its scratch or its class count before anything else
    for mode, ws in ((ATOMICS, 0), (FX, 0), (SLAB, BIG), (SLAB, 0), (SLAB, -1), (3, 0), (-1, 0)):
        out += [(CLASS_LOGITS,) + a + (mode, al, ws) for a in CL_REFUSED + [(7, 64, 196, 80), (0, 64, 196, 80)] for al in (1, 0)]
    return out


def table(L):
    plan, calls = plan_of(L), rows()
    ops = np.array([c[0] for c in calls], dtype=np.int32)
    args = np.array([c[1:] + (0,) * (8 - len(c)) for c in calls], dtype=np.int64)
    got = [plan(op, a) for op, a in zip(ops.tolist(), args.tolist())]
    return ops, args, np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=np.int32)


def check(L, path):
    t = np.load(path)
    plan, bad = plan_of(L), 0
    for op, a, rc, rec in zip(t['op'].tolist(), t['args'].tolist(), t['rc'].tolist(), t['rec'].tolist()):
        got = plan(op, a)
        if got != (rc, rec):
            bad += 1
            if bad <= 10:
                print('op', op, 'args', a[:COUNTS[op]], '\n  table  ', rc, rec, '\n  library', *got)
    print(f'{len(t["rc"])} rows, {bad} differ')
    return bad


def save(L, path):
    ops, args, rc, rec = table(L)
    np.savez_compressed(path, op=ops, args=args, rc=rc, rec=rec)
    print(f'{path}: {len(rc)} rows, {os.path.getsize(path)} bytes; return codes', dict(zip(*np.unique(rc, return_counts=True))))


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
        sys.exit(1 if check(L, o.check) else 0)
    save(L, o.out)


if __name__ == '__main__':
    main()
