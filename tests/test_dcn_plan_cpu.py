"""dm_deform_conv_plan: the DCN forward launcher's own route (csrc/deform_conv.hip: dcn_route, the value dcn_emit enqueues),
pinned at the 256-CU fallback of a machine without a device.  tests/golden/dcn_plan_256cu.npz is the routing of the launcher
as it was BEFORE it was restructured into validate / route / emit: recorded from that code with a recorder at each of its
launch sites, over a grid that crosses every threshold (tools/dcn_plan_table.py regenerates it from the current library; a
routing change is meant to show up as a diff of that table).  The hand-derived pins below carry their arithmetic in the
comment next to them: 256 CUs, two workgroups per CU -> 512 slots.  No GPU needed; on a machine WITH a device the
compute-unit count is the device's and the CU-dependent tests are skipped (tests/test_dcn_builds_gpu.py asks the plan there)."""
import ctypes
import os

import numpy as np
import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_DCN_PLAN_INTS'], CONSTS['DM_DCN_PLAN_MAX_LAUNCHES']
INVALID, UNSUPPORTED = CONSTS['DM_ERR_INVALID_ARG'], CONSTS['DM_ERR_UNSUPPORTED']
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dcn_plan_256cu.npz')
BIG = 1 << 40

GENERIC, LDS, C256, BAND = range(4)
T32x128 = dict(kernel=GENERIC, P0=1, P1=4, P2=1, P3=1, threads=256, lds_bytes=16 * 18 * (32 + 128))
T64x64 = dict(kernel=GENERIC, P0=2, P1=2, P2=1, P3=1, threads=256, lds_bytes=16 * 18 * (64 + 64))
T128x64 = dict(kernel=GENERIC, P0=2, P1=2, P2=2, P3=1, threads=256, lds_bytes=16 * 18 * (128 + 64))
NO_SPLIT = dict(ksplit=1, kchan=0, grid_y=1, reduce=0)


def band(wm, wgm, xr):
    return dict(kernel=BAND, P0=wm, P1=wgm, P2=xr, P3=0, threads=256, MT=1)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


needs_256 = pytest.mark.skipif(_cus() != 256, reason='pins worked out for the 256-CU count the library assumes without a device')


def _is(rec, build, **more):
    want = dict(build, **more)
    got = {k: rec[k] for k in want}
    assert got == want, (got, want)


def _raw(args, cap=N_REC, null=False, fill=-1):
    """dm_deform_conv_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([fill] * (N_INTS * N_REC)))
    rc = _lib.lib().dm_deform_conv_plan(*[int(v) for v in args], None if null else rec, cap)
    return rc, list(rec)


def test_record_layout_and_field_names():
    assert N_INTS == len(ops.DCN_PLAN_FIELDS) == 15 and N_REC == 2
    assert ops.DCN_KERNELS == ('generic', 'lds', 'c256', 'band')
    assert ops.deform_conv_plan(0, 256, 14, 14, 256, 1) == []            # NB = 0: DM_OK, nothing launched
    assert os.path.getsize(TABLE) < 1 << 20


@needs_256
def test_the_library_reproduces_the_recorded_table_row_for_row():
    t = np.load(TABLE)
    args, rcs, recs = t['args'], t['rc'], t['rec']
    assert len(args) == len(rcs) == len(recs) > 90000 and recs.shape[1] == N_INTS * N_REC
    bad = []
    for a, rc, rec in zip(args.tolist(), rcs.tolist(), recs.tolist()):
        got = _raw(a)
        if got != (rc, rec):
            bad.append((a, (rc, rec), got))
    assert not bad, (len(bad), bad[:3])
    # the table does cross the routes: every build, both seams, every split count, every return code
    first = recs[rcs >= 1][:, :N_INTS]
    builds = {tuple(r[:5]) for r in first.tolist()}
    assert len(builds) == 13
    assert {tuple(r[:5]) for r in recs[rcs == 2][:, :N_INTS].tolist()} == {(LDS, 0, 0, 0, 0), (C256, 0, 0, 0, 0)}
    assert set(first[:, 11].tolist()) == set(range(1, 9))
    assert {int(r[0]) for r in first[first[:, 11] > 1]} == {GENERIC, LDS, BAND}
    assert set(rcs.tolist()) == {INVALID, UNSUPPORTED, 0, 1, 2}


@needs_256
def test_headline_c256_main_launch_and_64x64_tail():
    # 512 x 256 x 14 x 14 -> 256: Q = 100352 = 1568 tiles of 64 px, one workgroup per tile holds the 256 couts.  1568 = 3 x 512 +
    # 32: three full rounds, rem = 32, 32 x 20 = 640 <= 3 x 512 -> the seam.  Main: 1536 workgroups = 98304 px, LDS 16 x (2 x 3 x
    # 2 x 64) + 4 x 2 x 2 x 8 x 196 = 12288 + 25088; the last 2048 px: 32 tiles of 64 px x MT 4 (256 / 64 couts) of the 64 x 64 build.
    main, tail = ops.deform_conv_plan(512, 256, 14, 14, 256, 1)
    _is(main, dict(kernel=C256, P0=0, P1=0, P2=0, P3=0, threads=256, MT=1), q_begin=0, Q=98304, grid_x=1536, lds_bytes=37376, **NO_SPLIT)
    _is(tail, T64x64, MT=4, q_begin=98304, Q=100352, grid_x=128, **NO_SPLIT)
    assert 98304 % 196 != 0 and 98304 // 196 == 501                      # the seam lies inside RoI 501
    # flag bit 3 (the caller overlaps another stream): one launch; ReLU and the deformable groups do not enter the route
    one, = ops.deform_conv_plan(512, 256, 14, 14, 256, 1, overlapped=True)
    _is(one, dict(kernel=C256), q_begin=0, Q=100352, grid_x=1568, **NO_SPLIT)
    assert ops.deform_conv_plan(512, 256, 14, 14, 256, 4, relu=True) == [main, tail]
    # 250 couts are packed to 256: same route
    assert ops.deform_conv_plan(512, 256, 14, 14, 250, 1) == [main, tail]
    # 128 couts: the 128 x 128 LDS kernel, MT 1: 784 tiles = 512 + 272, 272 x 20 > 1536 -> no seam; 520 RoIs: 101920 px = 797 tiles
    # (796.25) = 512 + 285: none; 16 x 16 maps x 260 RoIs: 66560 px = 520 tiles = 512 + 8 -> seam at 512 tiles = 65536 px
    one, = ops.deform_conv_plan(512, 256, 14, 14, 128, 1)
    _is(one, dict(kernel=LDS, MT=1), Q=100352, grid_x=784, lds_bytes=49152 + 25088, **NO_SPLIT)
    main, tail = ops.deform_conv_plan(260, 256, 16, 16, 128, 1)
    _is(main, dict(kernel=LDS, MT=1), q_begin=0, Q=65536, grid_x=512, lds_bytes=49152 + 32768, **NO_SPLIT)
    _is(tail, T64x64, MT=2, q_begin=65536, Q=66560, grid_x=2 * 16, **NO_SPLIT)


@needs_256
def test_37_rois_take_64x64_tiles_and_38_the_c256_kernel():
    # small launch: MT128 x ceil(Q / 128) x 20 <= 9 x 256 = 2304 with MT128 = 2 <=> ceil(Q / 128) <= 57.
    # 37 RoIs: 7252 px = 57 tiles (56.7) -> 64 x 64: MT 4 x 114 tiles of 64 px (113.3); 38 RoIs: 7448 px = 59 tiles (58.2) -> c256,
    # 117 tiles of 64 px (116.4)
    one, = ops.deform_conv_plan(37, 256, 14, 14, 256, 1)
    _is(one, T64x64, MT=4, q_begin=0, Q=7252, grid_x=456, **NO_SPLIT)
    one, = ops.deform_conv_plan(38, 256, 14, 14, 256, 1)
    _is(one, dict(kernel=C256, MT=1), q_begin=0, Q=7448, grid_x=117, **NO_SPLIT)
    # 224 couts (CoutP 224, MT128 still 2): the LDS kernel from 38 RoIs on, 2 x 59 workgroups
    _is(ops.deform_conv_plan(37, 256, 14, 14, 224, 1)[0], T64x64, MT=4, grid_x=456)
    _is(ops.deform_conv_plan(38, 256, 14, 14, 224, 1)[0], dict(kernel=LDS, MT=2), grid_x=118, **NO_SPLIT)
    # 128 couts (MT128 = 1): ceil(Q / 128) <= 115 <=> 75 RoIs (14700 px = 115 tiles (114.8)); 76: 14896 px = 117 tiles
    _is(ops.deform_conv_plan(75, 256, 14, 14, 128, 1)[0], T64x64, MT=2, grid_x=2 * 230)
    _is(ops.deform_conv_plan(76, 256, 14, 14, 128, 1)[0], dict(kernel=LDS, MT=1), grid_x=117)


@needs_256
def test_a_workspace_keeps_small_launches_on_the_lds_kernel_and_splits_them():
    per = lambda nb: nb * 256 * 196
    # 16 RoIs: 3136 px = 25 tiles of 128 (24.5) x MT 2 = 50 workgroups.  <= 24 RoIs: min(8, 512 / 50 = 10, 32 chunks / 2) = 8 splits
    # allowed; the model: 32 x 3.5 us x (1 - 1/S) saved, 5 + (S + 1) x 3.21 MB x 0.25 paid; its gain still grows at S = 8 (112 / 64 =
    # 1.75 us per step against 0.80): 98 - 12.2 = 85.8 us -> 8 splits of 4 chunks = 32 channels
    one, = ops.deform_conv_plan(16, 256, 14, 14, 256, 1, workspace_floats=8 * per(16))
    _is(one, dict(kernel=LDS, MT=2), q_begin=0, Q=3136, grid_x=50, grid_y=8, ksplit=8, kchan=32, reduce=1, lds_bytes=74240)
    # room for five copies: 5 splits of ceil(32 / 5) = 7 chunks -> ceil(32 / 7) = 5
    _is(ops.deform_conv_plan(16, 256, 14, 14, 256, 1, workspace_floats=6 * per(16) - 1)[0], dict(kernel=LDS), ksplit=5, kchan=56, grid_y=5)
    # room for one: no split, and then the c256 kernel (a workspace keeps the launch off the 64 x 64 tiles)
    _is(ops.deform_conv_plan(16, 256, 14, 14, 256, 1, workspace_floats=2 * per(16) - 1)[0], dict(kernel=C256, MT=1), grid_x=49, **NO_SPLIT)
    _is(ops.deform_conv_plan(16, 256, 14, 14, 256, 1)[0], T64x64, MT=4, grid_x=4 * 49)
    # 100 RoIs: 19600 px = 154 tiles (153.1) x 2 = 308 workgroups < 512, 32 chunks >= 12 -> three splits of 11 chunks = 88 channels
    one, = ops.deform_conv_plan(100, 256, 14, 14, 256, 1, workspace_floats=3 * per(100))
    _is(one, dict(kernel=LDS, MT=2), Q=19600, grid_x=308, grid_y=3, ksplit=3, kchan=88, reduce=1)
    # one float less: none, the c256 kernel (307 tiles of 64 px (306.25), less than a round: no seam)
    one, = ops.deform_conv_plan(100, 256, 14, 14, 256, 1, workspace_floats=3 * per(100) - 1)
    _is(one, dict(kernel=C256, MT=1), grid_x=307, **NO_SPLIT)
    # 128 / 129 RoIs: 25088 px = 196 tiles, 392 workgroups < 512 -> 3; 167 RoIs: 32732 px = 256 tiles (255.7), 512 workgroups: none
    assert ops.deform_conv_plan(129, 256, 14, 14, 256, 1, workspace_floats=BIG)[0]['ksplit'] == 3
    _is(ops.deform_conv_plan(167, 256, 14, 14, 256, 1, workspace_floats=BIG)[0], dict(kernel=C256), grid_x=512, **NO_SPLIT)
    # 16 input channels: 2 chunks, 2 / 2 = 1 split -> none
    _is(ops.deform_conv_plan(16, 16, 14, 14, 256, 1, workspace_floats=BIG)[0], dict(kernel=C256), **NO_SPLIT)


@needs_256
def test_band_kernel_few_boundary_on_28x28_and_128_couts():
    # 28 x 28 = 784 px = 7 tiles of 128 (6.1); few <=> NB x 7 x 4 < 3 x 256 = 768 <=> NB <= 27.  W = 28: 8 x 16 x 28 / 4 = 896 <= 1024
    # staging positions: narrow (XR 4).  LDS: 16 x (9 x 2 x 4 x 32) operand rings + 4 x 8 x 16 x 28 band planes = 36864 + 14336.
    # few: one cout tile per wave, 32 px per workgroup: 25 tiles (24.5) per image; else a wave holds all 128 couts of 32 px: 7 per image
    one, = ops.deform_conv_plan(27, 128, 28, 28, 128, 1)
    _is(one, band(1, 4, 4), q_begin=0, Q=27 * 784, grid_x=27 * 25, lds_bytes=51200, **NO_SPLIT)
    one, = ops.deform_conv_plan(28, 128, 28, 28, 128, 1)
    _is(one, band(4, 1, 4), q_begin=0, Q=28 * 784, grid_x=28 * 7, lds_bytes=51200, **NO_SPLIT)
    # 64 couts: <1, 2, 4> (64 px per workgroup: 13 tiles (12.25)) / <2, 1, 4>
    _is(ops.deform_conv_plan(27, 128, 28, 28, 64, 1)[0], band(1, 2, 4), grid_x=27 * 13, lds_bytes=18432 + 14336)
    _is(ops.deform_conv_plan(28, 128, 28, 28, 64, 1)[0], band(2, 1, 4), grid_x=28 * 7, lds_bytes=18432 + 14336)
    # a workspace and <= 24 RoIs: the full layout with its K loop split.  16 RoIs: 112 workgroups, min(8, 512 / 112 = 4, 16 chunks / 2)
    # = 4; per = 16 x 128 x 784 = 6.42 MB: 56 us x 3/4 - (5 + 5 x 1.61) = 29.0 us (three: 37.3 - 11.4 = 25.9) -> 4 splits of 4 chunks
    one, = ops.deform_conv_plan(16, 128, 28, 28, 128, 1, workspace_floats=BIG)
    _is(one, band(4, 1, 4), grid_x=112, grid_y=4, ksplit=4, kchan=32, reduce=1)
    _is(ops.deform_conv_plan(25, 128, 28, 28, 128, 1, workspace_floats=BIG)[0], band(1, 4, 4), **NO_SPLIT)       # (25 RoIs: few again)
    # the band kernel takes every batch of its maps: never the LDS or generic kernels, at 1 RoI or 1000
    for nb in (1, 1000):
        assert ops.deform_conv_plan(nb, 128, 28, 28, 128, 1)[0]['kernel'] == BAND


@needs_256
def test_band_kernel_narrow_and_wide_staging_w32_and_w36():
    # W = 32: 8 x 16 x 32 / 4 = 1024 <= 4 x 256 -> XR 4; W = 36: 1152 -> XR 7 (up to W = 56: 1792 = 7 x 256)
    # 16 x 32 = 512 px = 4 tiles: few <=> NB x 16 < 768 <=> NB <= 47; 16 x 36 = 576 px = 5 tiles (4.5): NB x 20 < 768 <=> NB <= 38
    _is(ops.deform_conv_plan(47, 64, 16, 32, 64, 1)[0], band(1, 2, 4), grid_x=47 * 8)
    _is(ops.deform_conv_plan(48, 64, 16, 32, 64, 1)[0], band(2, 1, 4), grid_x=48 * 4, lds_bytes=18432 + 16384)
    _is(ops.deform_conv_plan(38, 64, 16, 36, 64, 1)[0], band(1, 2, 7), grid_x=38 * 9)
    _is(ops.deform_conv_plan(39, 64, 16, 36, 64, 1)[0], band(2, 1, 7), grid_x=39 * 5, lds_bytes=18432 + 18432)
    # 128 couts: narrow maps let a wave hold all of them (<4, 1, 4>), wide ones share a pixel column between two waves
    # (<2, 2, 7>, 64 px per workgroup: 9 tiles)
    _is(ops.deform_conv_plan(48, 64, 16, 32, 128, 1)[0], band(4, 1, 4), grid_x=48 * 4)
    _is(ops.deform_conv_plan(39, 64, 16, 36, 128, 1)[0], band(2, 2, 7), grid_x=39 * 9, lds_bytes=36864 + 18432)
    _is(ops.deform_conv_plan(38, 64, 16, 36, 128, 1)[0], band(1, 4, 7), grid_x=38 * 18)
    # not band maps: W = 16 / 24 (a 128-px tile spans 9 / 7 rows: (16 - 9) / 2, (16 - 7) / 2 < 5 rows of margin), W = 60 (> 56),
    # H = 15, W = 30 (not a multiple of 4), 33 .. 64 couts only above 32
    for H, W in ((16, 16), (16, 24), (20, 60), (15, 28), (16, 30)):
        assert ops.deform_conv_plan(48, 64, H, W, 64, 1)[0]['kernel'] != BAND, (H, W)
    assert ops.deform_conv_plan(48, 64, 16, 28, 32, 1)[0]['kernel'] == GENERIC
    assert ops.deform_conv_plan(48, 64, 16, 28, 129, 1)[0]['kernel'] == GENERIC


@needs_256
def test_generic_builds_by_cout_on_7x7():
    # 2 RoIs of 7 x 7: 98 px.  <= 32 couts: 32 x 128 tiles (1 workgroup); 33 .. 64: 64 x 64 (2); 65: CoutP 96, a small launch (1 x 1 x 20 <=
    # 2304): 64 x 64, MT 2 x 2 tiles
    _is(ops.deform_conv_plan(2, 16, 7, 7, 32, 1)[0], T32x128, MT=1, q_begin=0, Q=98, grid_x=1, **NO_SPLIT)
    _is(ops.deform_conv_plan(2, 16, 7, 7, 33, 1)[0], T64x64, MT=1, Q=98, grid_x=2, **NO_SPLIT)
    _is(ops.deform_conv_plan(2, 16, 7, 7, 64, 1)[0], T64x64, MT=1, Q=98, grid_x=2, **NO_SPLIT)
    _is(ops.deform_conv_plan(2, 16, 7, 7, 65, 1)[0], T64x64, MT=2, Q=98, grid_x=4, **NO_SPLIT)
    # 65 .. 128 couts leave the 64 x 64 tiles where ceil(Q / 128) > 115: 300 RoIs = 14700 px = 115 tiles (114.8), 301 = 14749 px = 116
    # (115.2) -> 128 x 64: 231 tiles of 64 px (230.5).  (49 px: no LDS map, whatever the batch.)
    _is(ops.deform_conv_plan(300, 16, 7, 7, 65, 1)[0], T64x64, MT=2, grid_x=2 * 230)
    _is(ops.deform_conv_plan(301, 16, 7, 7, 65, 1)[0], T128x64, MT=1, Q=14749, grid_x=231, **NO_SPLIT)
    # 256 couts: MT128 = 2 -> ceil(Q / 128) <= 57: 148 RoIs = 7252 px = 57 tiles, 151 = 7399 px = 58 -> 128 x 64, MT 2 x 116 tiles
    _is(ops.deform_conv_plan(148, 16, 7, 7, 256, 1)[0], T64x64, MT=4)
    _is(ops.deform_conv_plan(151, 16, 7, 7, 256, 1)[0], T128x64, MT=2, grid_x=2 * 116)
    # these builds split too with a workspace: 2 RoIs x 256 channels x 64 couts, 2 workgroups: min(8, 256, 16) = 8 splits of 4 chunks
    _is(ops.deform_conv_plan(2, 256, 7, 7, 64, 1, workspace_floats=BIG)[0], T64x64, grid_x=2, grid_y=8, ksplit=8, kchan=32, reduce=1)


@needs_256
def test_the_workspace_bound_and_the_plan_agree():
    """What nothing checked before: dm_deform_conv_splitk_floats is an upper bound the route honours."""
    L = _lib.lib()
    t = np.load(TABLE)
    shapes = sorted({tuple(a[:5]) for a, rc in zip(t['args'].tolist(), t['rc'].tolist()) if rc >= 1 and a[5] == 1 and a[8] == 0})
    assert len(shapes) > 9000
    splits = 0
    for nb, c, H, W, cout in shapes:
        want = L.dm_deform_conv_splitk_floats(nb, c, H, W, cout)
        per = nb * cout * H * W
        for overlapped in (False, True):
            big = ops.deform_conv_plan(nb, c, H, W, cout, 1, overlapped=overlapped, workspace_floats=BIG)
            if overlapped:
                assert len(big) == 1, 'flag bit 3: no seam'
            if want == 0:
                assert all(r['ksplit'] == 1 and r['reduce'] == 0 for r in big), (nb, c, H, W, cout)
                continue
            got = ops.deform_conv_plan(nb, c, H, W, cout, 1, overlapped=overlapped, workspace_floats=want)
            assert got == big, 'more workspace than dm_deform_conv_splitk_floats changes the plan'
            assert got[0]['ksplit'] * per <= want
            for r in got:
                assert r['grid_y'] == r['ksplit'] and (r['kchan'] > 0) == (r['ksplit'] > 1) == bool(r['reduce'])
                if r['ksplit'] > 1:
                    splits += 1
                    assert len(got) == 1 and r['q_begin'] == 0 and r['Q'] == nb * H * W, 'a split launch has no seam'
                    assert r['kchan'] % 8 == 0 and (r['ksplit'] - 1) * r['kchan'] < c <= r['ksplit'] * r['kchan']
                    # it never needs more than it was given: the same split with exactly its own need, one float less: a smaller one
                    assert ops.deform_conv_plan(nb, c, H, W, cout, 1, overlapped=overlapped, workspace_floats=r['ksplit'] * per) == got
                    less = ops.deform_conv_plan(nb, c, H, W, cout, 1, overlapped=overlapped, workspace_floats=r['ksplit'] * per - 1)
                    assert less[0]['ksplit'] < r['ksplit']
        # two launches: the second begins where the first ends, and is the 64 x 64 build
        two = ops.deform_conv_plan(nb, c, H, W, cout, 1)
        if len(two) == 2:
            assert two[0]['q_begin'] == 0 and two[0]['Q'] == two[1]['q_begin'] and two[1]['Q'] == nb * H * W
            _is(two[1], T64x64, **NO_SPLIT)
    assert splits > 500


@needs_256
def test_tout_supported_is_the_plan_with_that_m2():
    L = _lib.lib()
    t = np.load(TABLE)
    seen = set()
    for a, rc in zip(t['args'].tolist(), t['rc'].tolist()):
        nb, c, H, W, cout, dg, flags, ws, m2 = a
        if m2 > 0 and dg == 1 and nb > 0:
            assert bool(L.dm_deform_conv_tout_supported(nb, c, H, W, cout, m2)) == (rc >= 1), a
            seen.add(rc >= 1)
            if rc >= 1:
                # ... and then the launch is the plain call's: the band build whose waves hold every cout
                one, = ops.deform_conv_plan(nb, c, H, W, cout, 1, m2=m2)
                assert one == ops.deform_conv_plan(nb, c, H, W, cout, 1, relu=True)[0]
                assert one['kernel'] == BAND and one['P1'] == 1 and one['P0'] * 32 == cout
    assert seen == {True, False}
    # 64 couts: M2 up to 32 (one 32-column block per two cout blocks, rounded up); 128 couts: up to 64, on narrow maps only;
    # never in the few-RoI layout (28 x 28: from 28 RoIs), never with Cout != C
    for args, ok in (((28, 64, 28, 28, 64, 32), 1), ((28, 64, 28, 28, 64, 33), 0), ((28, 128, 28, 28, 128, 64), 1),
                     ((28, 128, 28, 28, 128, 65), 0), ((27, 64, 28, 28, 64, 32), 0), ((39, 128, 16, 36, 128, 64), 0),
                     ((39, 64, 16, 36, 64, 32), 1), ((28, 256, 28, 28, 64, 32), 0), ((28, 64, 14, 14, 64, 32), 0),
                     ((28, 64, 28, 28, 64, 0), 0), ((0, 64, 28, 28, 64, 32), 0)):
        assert L.dm_deform_conv_tout_supported(*args) == ok, args
    assert _raw((28, 64, 28, 28, 64, 1, 0, BIG, 32))[0] == INVALID          # the chained call takes no workspace


ERRORS = [
    ('C % deform_groups', dict(dg=3), INVALID),
    ('no deformable group', dict(dg=0), INVALID),
    ('group channels not a multiple of 8', dict(dg=64), UNSUPPORTED),
    ('C = 20', dict(C=20), UNSUPPORTED),
    ('W = 1', dict(W=1), UNSUPPORTED),
    ('W = 1 and NB = 0', dict(W=1, NB=0), UNSUPPORTED),
    ('group channels and NB = 0', dict(C=20, NB=0), UNSUPPORTED),
    ('bf16x3', dict(flags=16), UNSUPPORTED),
    ('bf16x3 before the arguments', dict(flags=17, dg=3, NB=-1), UNSUPPORTED),
    ('NB < 0', dict(NB=-1), INVALID),
    ('H = 0', dict(H=0), INVALID),
    ('W = 0', dict(W=0), INVALID),
    ('Cout = 0', dict(cout=0), INVALID),
    ('invalid before unsupported', dict(W=1, cout=0), INVALID),
    ('2^31 pixels', dict(NB=1 << 20, H=64, W=32), INVALID),
    ('negative workspace', dict(ws=-1), INVALID),
    ('negative M2', dict(m2=-1), INVALID),
    ('one record of room', dict(cap=1), INVALID),
    ('null record array', dict(null=True), INVALID),
]


@pytest.mark.parametrize('name,change,code', ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_return_their_code_and_write_nothing(name, change, code):
    base = dict(NB=512, C=256, H=14, W=14, cout=256, dg=1, flags=0, ws=0, m2=0)
    order = ('NB', 'C', 'H', 'W', 'cout', 'dg', 'flags', 'ws', 'm2')
    ok, rec = _raw([base[k] for k in order], fill=-77)
    assert ok >= 1 and rec[ok * N_INTS:] == [-77] * ((N_REC - ok) * N_INTS) and -77 not in rec[:ok * N_INTS]
    call = dict(base, **change)
    rc, rec = _raw([call[k] for k in order], cap=call.get('cap', N_REC), null=call.get('null', False), fill=-77)
    assert rc == code, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'


def test_nb_0_is_ok_after_the_argument_checks():
    assert _raw((0, 256, 14, 14, 256, 1, 0, 0, 0))[0] == 0
    assert _raw((0, 256, 14, 14, 256, 1, 0, BIG, 0))[0] == 0
    assert _raw((0, 256, 14, 14, 256, 3, 0, 0, 0))[0] == INVALID
    # the chained call answers NB = 0 first, then for its shape, then for its arguments
    assert _raw((0, 256, 14, 14, 256, 3, 0, 0, 30))[0] == 0
    assert _raw((5, 256, 14, 14, 256, 3, 0, 0, 30))[0] == UNSUPPORTED
    with pytest.raises(RuntimeError, match='dm_deform_conv_plan'):
        ops.deform_conv_plan(5, 256, 14, 1, 256, 1)
