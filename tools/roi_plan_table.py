"""Dump dm_roi_align_plan over a grid that crosses every threshold of the RoIAlign launchers (csrc/roi_align.hip: roi_route):
tests/golden/roi_plan.npz, which tests/test_roi_plan_cpu.py replays row for row.  No device needed, whatever its size: the
route reads no compute-unit count.

    python tools/roi_plan_table.py [--out FILE]           # regenerate from the current library
    python tools/roi_plan_table.py --check [FILE]         # compare the current library with a table, print the first differences

Arrays: ``args`` int64 [N, 21] = entry, pool, num_levels, H[0..4], W[0..4], B, C, N, P, sampling_ratio, workspace_bytes,
workspace (0 none, 1 aligned, 2 misaligned), knobs (index into KNOBS: the environment the row is planned under, set through
dm_reload_env_knobs); ``rc`` int32 [N] the return code (launches, or the negative error); ``rec`` int32 [N, 2 *
DM_ROI_PLAN_INTS] the records, -1 where nothing is written.  A routing change is meant to show up here: regenerate, and
read the diff of the table before committing it."""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamask_amd import _abi, _lib  # noqa: E402

DEFAULT = os.path.join(ROOT, 'tests', 'golden', 'roi_plan.npz')
CONSTS = _abi.load()[1]
N_INTS, N_REC, MAX_LEVELS = CONSTS['DM_ROI_PLAN_INTS'], CONSTS['DM_ROI_PLAN_MAX_LAUNCHES'], CONSTS['DM_MAX_LEVELS']
FWD, ADD, BWD = range(3)
KNOBS = ({}, {'DM_ROI_SORT': '0'}, {'DM_ROI_SORT_MIN': '1'})

PS = [1, 2, 7, 11, 14, 16, 17, 28, 56, 64, 65, 112]
CS = [3, 4, 16, 64, 100, 128, 256, 260]
NS = [0, 1, 191, 192, 193, 1024, 1025, 4096]
PYRAMID = ((200, 100, 50, 25), (336, 168, 84, 42))                 # the FPN maps of a 1333 x 800 image
ONE = ((200,), (336,))
# one level of 2^23 pixels that the band kernel takes too (W < 2^20); 2^23 + 1 = 3 x 2796203; 2^23 with W = 2^20; W = 2^20 - 1
EDGE_MAPS = [((16,), (1 << 19,)), ((2796203,), (3,)), ((8,), (1 << 20,)), ((1,), ((1 << 20) - 1,)),
             ((200, 100, 16, 25), (336, 168, 1 << 19, 42)), ((200, 100, 50, 2796203), (336, 168, 84, 3))]


def row(entry, maps, B, C, N, P, sr=0, ws_bytes=0, ws=0, pool=0, knobs=0, levels=None):
    H, W = maps
    L = len(H) if levels is None else levels
    pad = lambda v: list(v)[:5] + [1] * (5 - len(v))               # noqa: E731  (five slots: num_levels = DM_MAX_LEVELS + 1)
    return [entry, pool, L, *pad(H), *pad(W), B, C, N, P, sr, ws_bytes, ws, knobs]


def workspaces(N):
    """absent; one byte short, exact, more than enough; misaligned; bytes without a pointer"""
    need = 32 * N
    return [(0, 0), (need - 1, 1), (need, 1), (need + 4096, 1), (need, 2), (need, 0), (0, 1)]


def rows():
    out = []
    for k in range(len(KNOBS)):
        # the forward: every P x C x N on the pyramid with every workspace; the single map and the edge maps on a thinner grid
        for P in PS:
            for C in CS:
                for N in NS:
                    for b, w in workspaces(N):
                        out.append(row(FWD, PYRAMID, 2, C, N, P, ws_bytes=b, ws=w, knobs=k))
                    out.append(row(FWD, ONE, 2, C, N, P, knobs=k))
                    out.append(row(FWD, ONE, 2, C, N, P, ws_bytes=32 * N, ws=1, knobs=k))
                    out.append(row(BWD, PYRAMID, 2, C, N, P, knobs=k))
                    out.append(row(BWD, ONE, 1, C, N, P, knobs=k))
                    for pool in (1, 2):
                        out.append(row(ADD, ONE, 2, C, N, P, pool=pool, knobs=k))
            for maps in EDGE_MAPS:
                for C in (3, 4, 256):
                    for N in (0, 1, 192, 1024):
                        out.append(row(FWD, maps, 1, C, N, P, knobs=k))
                        out.append(row(FWD, maps, 1, C, N, P, ws_bytes=32 * N, ws=1, knobs=k))
                        out.append(row(BWD, maps, 1, C, N, P, knobs=k))
                        if len(maps[0]) == 1:
                            out.append(row(ADD, maps, 1, C, N, P, pool=1 + (N & 1), knobs=k))
            # the add entry: N x chunks at and beyond 2^31 (16 chunks of 16 channels), odd / even P with both pools above
            for N in ((1 << 27) - 1, 1 << 27):
                for C in (16, 256):
                    out.append(row(ADD, ONE, 2, C, N, P, pool=1, knobs=k))
    # sampling ratios, level counts, and the refused calls alone and in pairs (the precedence of the checks)
    for entry in (FWD, ADD, BWD):
        one = entry == ADD
        for P in PS:
            for sr in (-1, 0, 2):
                for N in (0, 192):
                    for C in (4, 6):
                        out.append(row(entry, ONE if one else PYRAMID, 2, C, N, P, sr=sr, pool=2 if one else 0))
        for P in (-1, 0, 7, 14, 28, 112):
            for N in (-1, 0, 5, 200):
                for pool in ((0, 1, 2, 3) if one else (0,)):
                    for B, C in ((2, 256), (0, 256), (2, 0), (2, -4), (-1, 6)):
                        out.append(row(entry, ONE if one else PYRAMID, B, C, N, P, pool=pool))
                if not one:
                    for levels in (0, 1, 2, MAX_LEVELS, MAX_LEVELS + 1, -1):
                        out.append(row(entry, ((200, 100, 50, 25, 13), (336, 168, 84, 42, 21)), 2, 256, N, P, levels=levels))
                for maps in (((200, 0, 50, 25), (336, 168, 84, 42)), ((200, 100, 50, 25), (336, 168, 84, -1)), ((0,), (336,)), ((200,), (0,))):
                    if one == (len(maps[0]) == 1):
                        out.append(row(entry, maps, 2, 256, N, P, pool=1 if one else 0))
    return out


def set_knobs(L, k):
    for name in ('DM_ROI_SORT', 'DM_ROI_SORT_MIN'):
        os.environ.pop(name, None)
    os.environ.update(KNOBS[k])
    L.dm_reload_env_knobs()


def plan(L, a):
    """One row through dm_roi_align_plan (the knobs are the caller's to set): (rc, the record ints)."""
    a = [int(v) for v in a]
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([-1] * (N_INTS * N_REC)))
    rc = L.dm_roi_align_plan(a[0], a[1], a[2], (ctypes.c_int * 5)(*a[3:8]), (ctypes.c_int * 5)(*a[8:13]), *a[13:20], rec, N_REC)
    return rc, list(rec)


def replay(L, args, each):
    """each(i, rc, rec) for every row of ``args`` as the current library plans it, knobs set per row and put back after."""
    was = {n: os.environ.get(n) for n in ('DM_ROI_SORT', 'DM_ROI_SORT_MIN')}
    try:
        cur = None
        for i, a in enumerate(args):
            if a[20] != cur:
                cur = int(a[20])
                set_knobs(L, cur)
            each(i, *plan(L, a))
    finally:
        for n, v in was.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v
        L.dm_reload_env_knobs()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=DEFAULT)
    ap.add_argument('--check', nargs='?', const=DEFAULT)
    o = ap.parse_args()
    L = _lib.lib()
    if o.check:
        t = np.load(o.check)
        bad = []

        def each(i, rc, rec):
            if (rc, rec) != (int(t['rc'][i]), t['rec'][i].tolist()):
                bad.append(i)
                if len(bad) <= 10:
                    print('args', t['args'][i].tolist(), '\n  table  ', int(t['rc'][i]), t['rec'][i].tolist(), '\n  library', rc, rec)
        replay(L, t['args'].tolist(), each)
        print(f'{len(t["rc"])} rows, {len(bad)} differ')
        sys.exit(1 if bad else 0)
    args = rows()
    rcs, recs = [], []
    replay(L, args, lambda i, rc, rec: (rcs.append(rc), recs.append(rec)))
    np.savez_compressed(o.out, args=np.array(args, dtype=np.int64), rc=np.array(rcs, dtype=np.int32), rec=np.array(recs, dtype=np.int32))
    print(f'{o.out}: {len(rcs)} rows, {os.path.getsize(o.out)} bytes; return codes', dict(zip(*np.unique(rcs, return_counts=True))))


if __name__ == '__main__':
    main()
