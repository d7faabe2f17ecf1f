"""dm_conv2d_wgrad_plan: the weight-gradient launcher's own route (csrc/backward.hip: wgrad_route, the value wgrad_emit
enqueues), pinned at the 256-CU fallback of a machine without a device.  tests/golden/wgrad_plan_256cu.npz is the routing of
the launcher as it was BEFORE it was restructured into validate / route / emit: recorded from that code with a recorder at
each of its thirteen launch sites, over a grid that crosses every threshold (tools/wgrad_plan_table.py regenerates it from
the current library; a routing change is meant to show up as a diff of that table).  The hand-derived pins below carry their
arithmetic in the comment next to them: 256 CUs, two workgroups per CU -> a target of 512 workgroups.  No GPU needed; on a
machine WITH a device the compute-unit count is the device's and the CU-dependent tests are skipped
(tests/test_wgrad_builds_gpu.py asks the plan there)."""
import ctypes
import os

import numpy as np
import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_WGRAD_PLAN_INTS'], CONSTS['DM_WGRAD_PLAN_MAX_LAUNCHES']
INVALID = CONSTS['DM_ERR_INVALID_ARG']
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'wgrad_plan_256cu.npz')
BIG = 1 << 40
TARGET = 512
BOUND = TARGET * (16384 + 256)

GEMM, NARROW, REDUCE = range(3)
ATOMICS, SLAB, FX = range(3)
# args columns of the table (dm_conv2d_wgrad_plan's order)
DY_BS, COUT, X_BS, CS, NB, H, W, KS, BIAS, MODE, SCRATCH, IO8, S16 = range(13)
# record ints
R_KERNEL, R_MT, R_JT, R_SPLITS, R_SLABS, R_ROWS, R_STRIDE, R_ACCUM = 0, 9, 10, 11, 13, 15, 16, 17


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


needs_256 = pytest.mark.skipif(_cus() != 256 or bool(os.environ.get('DM_WGRAD_WGS')),
                               reason='pins worked out for the 256-CU count the library assumes without a device, DM_WGRAD_WGS unset')


def gemm(ks, wgm, wgn, wgk, tail=0):
    return dict(kernel=GEMM, P0=ks, P1=wgm, P2=wgn, P3=wgk, P4=tail, threads=256, lds_bytes=0)


def narrow(tail):
    return dict(kernel=NARROW, P0=3, P1=0, P2=0, P3=0, P4=tail, threads=256, MT=1)


def reduce_(p, grid, slabs, splits):
    return dict(kernel=REDUCE, P0=p, P1=0, P2=0, P3=0, P4=0, grid=grid, threads=256, lds_bytes=0, MT=0, JT=0, per_split=0, slabs=slabs,
                splits=splits, accum=SLAB)


def _is(rec, build, **more):
    want = dict(build, **more)
    got = {k: rec[k] for k in want}
    assert got == want, (got, want)


def _raw(args, cap=N_REC, null=False, fill=-1):
    """dm_conv2d_wgrad_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([fill] * (N_INTS * N_REC)))
    rc = _lib.lib().dm_conv2d_wgrad_plan(*[int(v) for v in args], None if null else rec, cap)
    return rc, list(rec)


def test_record_layout_and_field_names():
    assert N_INTS == len(ops.WGRAD_PLAN_FIELDS) == 18 and N_REC == 2
    assert ops.WGRAD_KERNELS == ('gemm', 'narrow', 'reduce') and ops.WGRAD_MODES == ('atomics', 'slab', 'fx')
    assert os.path.getsize(TABLE) < 1 << 20


@needs_256
def test_the_library_reproduces_the_recorded_table_row_for_row():
    t = np.load(TABLE)
    args, rcs, recs = t['args'], t['rc'], t['rec']
    assert len(args) == len(rcs) == len(recs) > 90000 and recs.shape[1] == N_INTS * N_REC and args.shape[1] == 13
    bad = []
    for a, rc, rec in zip(args.tolist(), rcs.tolist(), recs.tolist()):
        got = _raw(a)
        if got != (rc, rec):
            bad.append((a, (rc, rec), got))
    assert not bad, (len(bad), bad[:3])


@needs_256
def test_the_table_covers_the_routes():
    t = np.load(TABLE)
    args, rcs, recs = t['args'], t['rc'], t['rec']
    ok = rcs >= 1
    first, second = recs[ok][:, :N_INTS], recs[rcs == 2][:, N_INTS:]
    # every build the launcher can name: seven GEMM builds for each ksize, the narrow kernel with and without tail, every P
    seven = lambda ks: {(ks, 1, 4, 1, 1), (ks, 1, 4, 1, 0), (ks, 1, 2, 2, 1), (ks, 1, 2, 2, 0), (ks, 1, 1, 4, 0), (ks, 2, 2, 1, 0), (ks, 2, 1, 2, 0)}
    assert {tuple(r[1:6]) for r in first[first[:, R_KERNEL] == GEMM].tolist()} == seven(1) | seven(3)
    assert {tuple(r[1:6]) for r in first[first[:, R_KERNEL] == NARROW].tolist()} == {(3, 0, 0, 0, 0), (3, 0, 0, 0, 1)}
    assert set(second[:, R_KERNEL].tolist()) == {REDUCE} and {tuple(r[1:6]) for r in second.tolist()} == {(p, 0, 0, 0, 0) for p in (1, 4, 16, 64)}
    # both kernels in all three accumulations; the reduce follows exactly the launches that took slabs
    for kernel in (GEMM, NARROW):
        assert set(first[first[:, R_KERNEL] == kernel][:, R_ACCUM].tolist()) == {ATOMICS, SLAB, FX}
    assert ((first[:, R_ACCUM] == SLAB) == (rcs[ok] == 2)).all()
    assert (first[args[ok][:, MODE] == FX][:, R_ACCUM] == FX).all() and (first[args[ok][:, MODE] == ATOMICS][:, R_ACCUM] == ATOMICS).all()
    # slab calls that fell back to float atomics, for each of the three causes
    a, f = args[ok], first
    fell = (a[:, MODE] == SLAB) & (f[:, R_ACCUM] == ATOMICS)
    misaligned = fell & (a[:, S16] == 0)
    short = fell & (a[:, S16] == 1) & (a[:, SCRATCH] != BOUND)
    tiles = fell & (a[:, S16] == 1) & (a[:, SCRATCH] == BOUND)
    assert misaligned.sum() > 1000 and short.sum() > 1000 and tiles.sum() >= 10
    assert (f[tiles][:, R_MT] * f[tiles][:, R_JT] > TARGET).all() and (f[tiles][:, R_SPLITS] == 1).all()
    assert set(f[tiles][:, R_KERNEL].tolist()) == {GEMM}
    # the split count goes from 1 (the chunks limit it: 8 pixels are one chunk) to the target
    assert first[:, R_SPLITS].min() == 1 and first[:, R_SPLITS].max() == TARGET
    assert ((a[:, NB] * a[:, H] * a[:, W] <= 32) & (f[:, R_KERNEL] == GEMM) & (f[:, R_MT] * f[:, R_JT] == 1)).any()
    # the narrow kernel with one row band and with several; off it by each of its conditions
    k3 = (a[:, KS] == 3) & (a[:, COUT] <= 36)
    on = k3 & (f[:, R_KERNEL] == NARROW)
    assert not (on & ((a[:, W] % 2 == 1) | (a[:, W] < 8) | (a[:, IO8] == 0) | (a[:, DY_BS] % 2 == 1) | (a[:, X_BS] % 2 == 1))).any()
    even = k3 & (a[:, W] % 2 == 0) & (a[:, W] >= 8)
    for off in (even & (a[:, IO8] == 0), even & (a[:, DY_BS] % 2 == 1), even & (a[:, X_BS] % 2 == 1), even & (a[:, W] == 156)):
        assert off.sum() > 50 and (f[off][:, R_KERNEL] == GEMM).all()
    assert on[(a[:, W] == 14) | (a[:, W] == 28) | (a[:, W] == 64) | (a[:, W] == 150)].sum() > 1000
    assert not (f[:, R_KERNEL] == NARROW)[~k3].any()
    # every return code: one launch, two, and the refusal (a launch failure needs a device)
    assert set(rcs.tolist()) == {INVALID, 1, 2}
    assert (recs[rcs < 0] == -1).all() and (recs[rcs == 1][:, N_INTS:] == -1).all()


@needs_256
def test_conv3x3_256_to_256_at_14_with_256_rois():
    # TM 128 (256 couts > 64), MT 2.  J = 256 x 9 = 2304 columns: TN 128 costs 2304 x (1 + 32/128) = 2880, TN 64 costs 2304 x 1.5 =
    # 3456 -> TN 128, JT 18, build <3, 2, 2, 1>.  Q = 256 x 196 = 50176 px = 1568 chunks of 32; 36 tiles -> 512 / 36 = 14 splits of
    # 112 chunks; grid 36 x 14 = 504.  One K-wave: 14 slabs of 256 x 2304 floats.  Reduce: 14 slabs -> P 4, 64 quads per
    # workgroup: 256 x 576 quads / 64 = 2304 workgroups, + 256 / 32 = 8 for the bias.
    main, red = ops.conv2d_wgrad_plan(256, 256, 256, 14, 14, 3, has_bias=True)
    _is(main, gemm(3, 2, 2, 1), grid=504, MT=2, JT=18, splits=14, per_split=112, slabs=14, slab_ld=2304, slab_rows=256, slab_stride=589824,
        accum=SLAB)
    _is(red, reduce_(4, 2304 + 8, 14, 14), slab_ld=2304, slab_rows=256, slab_stride=589824)
    assert ops.conv2d_wgrad_plan(256, 256, 256, 14, 14, 3)[1]['grid'] == 2304                 # no bias: no bias workgroups
    # the same launch with atomics / in fixed point: one launch, no slabs
    for mode, accum in (('atomics', ATOMICS), ('fx', FX)):
        one, = ops.conv2d_wgrad_plan(256, 256, 256, 14, 14, 3, mode=mode, has_bias=True)
        _is(one, gemm(3, 2, 2, 1), grid=504, splits=14, per_split=112, slabs=0, slab_ld=0, slab_rows=0, slab_stride=0, accum=accum)


# tools/kbench.py's `wgrad` list: the training shapes, 256 RoIs, no bias.  (name, cin, cout, S, ks, main launch, reduce)
KBENCH = [
    # (the shape above without its bias)
    ('wgrad3x3 256->256 @14', 256, 256, 14, 3,
     dict(gemm(3, 2, 2, 1), grid=504, MT=2, JT=18, splits=14, per_split=112, slabs=14, slab_ld=2304, slab_rows=256, slab_stride=589824),
     reduce_(4, 2304, 14, 14)),
    # 36 couts, W 14 even: the narrow kernel, TAIL.  One band of 14 rows: x plane (16 x 15 + 1) | 1 = 241, dy row 196 | 1 = 197 floats:
    # 4 x (32 x 241 + 36 x 197) = 59216 B (<= 78 KB; the epilogue's 9 x 36 x 32 floats are less).  8 groups of 32 channels, 256 units
    # (image, band): min(256, 512 / 8) = 64 splits of 4 units, grid 512.  Slabs: 64 of 36 x (8 x 288); reduce P 4: 36 x 576 / 64 = 324
    ('wgrad3x3 256->36 @14', 256, 36, 14, 3,
     dict(narrow(1), grid=512, lds_bytes=59216, JT=8, splits=64, per_split=4, slabs=64, slab_ld=2304, slab_rows=36, slab_stride=82944),
     reduce_(4, 324, 64, 64)),
    # 56 x 56: rows of 57 / 56 floats.  R = 4: plane 6 x 57 + 1 = 343, dy row 225: 4 x (32 x 343 + 36 x 225) = 76304 B; R = 5: 4 x (32 x 401
    # + 36 x 281) = 91792 > 79872 -> 14 bands of 4 rows.  2 groups, 3584 units: min(3584, 256) = 256 splits of 14, grid 512.  Slabs:
    # 256 of 36 x 576; reduce P 16: 36 x 144 quads / 16 = 324
    ('wgrad3x3 64->36 @56', 64, 36, 56, 3,
     dict(narrow(1), grid=512, lds_bytes=76304, JT=2, splits=256, per_split=14, slabs=256, slab_ld=576, slab_rows=36, slab_stride=20736),
     reduce_(16, 324, 256, 256)),
    # the DCN's GEMMs over the column matrix.  2304 columns x 256 couts: the tiling of the 3x3 above
    ('wgrad1x1 2304->256 @14 (dcn)', 2304, 256, 14, 1,
     dict(gemm(1, 2, 2, 1), grid=504, MT=2, JT=18, splits=14, per_split=112, slabs=14, slab_ld=2304, slab_rows=256, slab_stride=589824),
     reduce_(4, 2304, 14, 14)),
    # 128 couts: MT 1; J 1152: TN 128 1440 < TN 64 1728 -> JT 9.  Q = 256 x 784 = 200704 = 6272 chunks; 512 / 9 = 56 splits of 112; grid
    # 504; 56 slabs of 128 x 1152 -> P 4: 128 x 288 / 64 = 576
    ('wgrad1x1 1152->128 @28 (dcn)', 1152, 128, 28, 1,
     dict(gemm(1, 2, 2, 1), grid=504, MT=1, JT=9, splits=56, per_split=112, slabs=56, slab_ld=1152, slab_rows=128, slab_stride=147456),
     reduce_(4, 576, 56, 56)),
    # 64 couts: TM 64.  J 576: TN 256 768 x 1.125 = 864, TN 128 640 x 1.25 = 800, TN 64 576 x 1.5 = 864 -> TN 128, JT 5, two K-waves.
    # Q = 256 x 3136 = 802816 = 25088 chunks; 512 / 5 = 102 splits of ceil(25088 / 102) = 246 -> ceil(25088 / 246) = 102; grid 510; 204 slabs
    # of 64 x 640 -> P 16: 64 x 144 / 16 = 576
    ('wgrad1x1 576->64 @56 (dcn)', 576, 64, 56, 1,
     dict(gemm(1, 1, 2, 2), grid=510, MT=1, JT=5, splits=102, per_split=246, slabs=204, slab_ld=640, slab_rows=64, slab_stride=40960),
     reduce_(16, 576, 204, 102)),
    # J 256, TM 128: TN 128 320 < TN 64 384 -> JT 2, 4 tiles: 128 splits of ceil(1568 / 128) = 13 -> ceil(1568 / 13) = 121; grid 484; 121
    # slabs of 256 x 256 -> P 16: 256 x 64 / 16 = 1024
    ('wgrad1x1 256->256 @14', 256, 256, 14, 1,
     dict(gemm(1, 2, 2, 1), grid=484, MT=2, JT=2, splits=121, per_split=13, slabs=121, slab_ld=256, slab_rows=256, slab_stride=65536),
     reduce_(16, 1024, 121, 121)),
    # one tile: 512 splits of ceil(6272 / 512) = 13 -> 483; 483 slabs of 128 x 128 -> P 64: 128 x 32 / 4 = 1024
    ('wgrad1x1 128->128 @28', 128, 128, 28, 1,
     dict(gemm(1, 2, 2, 1), grid=483, MT=1, JT=1, splits=483, per_split=13, slabs=483, slab_ld=128, slab_rows=128, slab_stride=16384),
     reduce_(64, 1024, 483, 483)),
    # J 64: TN 64 costs 96 (TN 128: 160, TN 256: 288): four K-waves.  25088 chunks / 512 = 49 exactly: 512 splits, 2048 slabs of 64 x 64
    # (with the bias rows 2048 x 4096 + 512 x 64 = 8421376 floats of the 8519680 the scratch has) -> P 64: 64 x 16 / 4 = 256
    ('wgrad1x1 64->64 @56', 64, 64, 56, 1,
     dict(gemm(1, 1, 1, 4), grid=512, MT=1, JT=1, splits=512, per_split=49, slabs=2048, slab_ld=64, slab_rows=64, slab_stride=4096),
     reduce_(64, 256, 2048, 512)),
    # 30 couts: the same launch; 30 x 16 / 4 = 120
    ('wgrad1x1 64->30 @56', 64, 30, 56, 1,
     dict(gemm(1, 1, 1, 4), grid=512, MT=1, JT=1, splits=512, per_split=49, slabs=2048, slab_ld=64, slab_rows=64, slab_stride=4096),
     reduce_(64, 120, 2048, 512)),
]


@needs_256
@pytest.mark.parametrize('name,cin,cout,S,ks,main,red', KBENCH, ids=[k[0] for k in KBENCH])
def test_training_shapes_of_kbench(name, cin, cout, S, ks, main, red):
    got = ops.conv2d_wgrad_plan(256, cout, cin, S, S, ks)
    assert len(got) == 2
    _is(got[0], main, accum=SLAB)
    _is(got[1], red, slab_ld=main['slab_ld'], slab_rows=main['slab_rows'], slab_stride=main['slab_stride'])


@needs_256
def test_tail_builds_and_narrow_eligibility():
    # 33 .. 36 couts on the GEMM (1x1, or a 3x3 the narrow kernel does not take): the TAIL twin of the 256- and 128-wide builds, the
    # plain 64-wide one.  J 256 -> TN 256 (288 < 320 < 384), J 128 -> TN 128 (160 < 192 < 288), J 64 -> TN 64
    _is(ops.conv2d_wgrad_plan(3, 36, 256, 7, 7, 1)[0], gemm(1, 1, 4, 1, 1), MT=1, JT=1)
    _is(ops.conv2d_wgrad_plan(3, 33, 128, 7, 7, 1)[0], gemm(1, 1, 2, 2, 1), MT=1, JT=1)
    _is(ops.conv2d_wgrad_plan(3, 33, 64, 7, 7, 1)[0], gemm(1, 1, 1, 4, 0), MT=1, JT=1)
    _is(ops.conv2d_wgrad_plan(3, 32, 256, 7, 7, 1)[0], gemm(1, 1, 4, 1, 0))
    _is(ops.conv2d_wgrad_plan(3, 37, 256, 7, 7, 1)[0], gemm(1, 1, 4, 1, 0))
    # 3x3, 36 couts, 24 channels (J 216 -> TN 256): a 7-wide map is the GEMM's, an 8-wide one the narrow kernel's -- unless dy or x
    # is not 8-byte aligned or a batch stride is odd
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 7, 7, 3)[0], gemm(3, 1, 4, 1, 1))
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 8, 8, 3)[0], narrow(1), JT=1)
    _is(ops.conv2d_wgrad_plan(3, 16, 24, 8, 8, 3)[0], narrow(0), JT=1)
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 8, 8, 3, io_aligned8=False)[0], gemm(3, 1, 4, 1, 1))
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 8, 8, 3, dy_bs=36 * 64 + 1)[0], gemm(3, 1, 4, 1, 1))
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 8, 8, 3, x_bs=24 * 64 + 1)[0], gemm(3, 1, 4, 1, 1))
    _is(ops.conv2d_wgrad_plan(3, 37, 24, 8, 8, 3)[0], gemm(3, 1, 4, 1, 0))
    # a row of 156: 4 x (32 x ((3 x 157 + 1) | 1) + 32 x (156 | 1)) = 4 x (32 x 473 + 32 x 157) = 80640 B > 79872: not one row fits
    _is(ops.conv2d_wgrad_plan(3, 32, 24, 2, 156, 3)[0], gemm(3, 1, 4, 1, 0))
    # 150: 4 x (32 x 455 + 36 x 151) = 79984 > 79872 with 36 rows of dy, 32 rows: 4 x (32 x 455 + 32 x 151) = 77568: one row per band
    _is(ops.conv2d_wgrad_plan(3, 36, 24, 2, 150, 3)[0], gemm(3, 1, 4, 1, 1))
    _is(ops.conv2d_wgrad_plan(3, 32, 24, 2, 150, 3)[0], narrow(0), lds_bytes=77568, splits=6, per_split=1)


@needs_256
def test_the_scratch_bound_and_the_plan_agree():
    """What nothing checked before: dm_conv2d_wgrad_scratch_floats() yields the slab route for every call with at most
    `target` output tiles -- and not for every shape, as the header used to say."""
    assert _lib.lib().dm_conv2d_wgrad_scratch_floats() == BOUND
    t = np.load(TABLE)
    shapes = sorted({tuple(a[:MODE]) for a, rc in zip(t['args'].tolist(), t['rc'].tolist()) if rc >= 1})
    assert len(shapes) > 15000
    over = 0
    for s in shapes:
        for io8 in (1, 0):
            rc, rec = _raw(s + (SLAB, BOUND, io8, 1))
            if rec[R_MT] * rec[R_JT] <= TARGET:
                assert rc == 2 and rec[R_ACCUM] == SLAB, s
                used = rec[R_SLABS] * rec[R_STRIDE] + rec[R_SPLITS] * rec[R_ROWS]
                assert used <= BOUND
                # it never needs more than it was given: the same route with exactly its own need, one float less: atomics
                assert _raw(s + (SLAB, used, io8, 1)) == (rc, rec)
                less = _raw(s + (SLAB, used - 1, io8, 1))
                assert less[0] == 1 and less[1][R_ACCUM] == ATOMICS and less[1][:R_SLABS] == rec[:R_SLABS]
            else:
                over += 1
                assert rec[R_SPLITS] == 1
                big = _raw(s + (SLAB, BIG, io8, 1))
                assert big[0] == 2 and big[1][:R_SLABS] == rec[:R_SLABS]
                used = big[1][R_SLABS] * big[1][R_STRIDE] + big[1][R_ROWS]
                assert (rc == 2) == (used <= BOUND), s
    assert over > 20
    # the header's example: 1024 -> 1024 channels 3x3: 8 x 72 = 576 tiles > 512: one split, one slab of 1024 x 9216 floats + 1024
    one, = ops.conv2d_wgrad_plan(1, 1024, 1024, 8, 8, 3, has_bias=True)
    _is(one, gemm(3, 2, 2, 1), grid=576, MT=8, JT=72, splits=1, slabs=0, accum=ATOMICS)
    assert 1024 * 9216 + 1024 == 9438208 > BOUND
    assert ops.conv2d_wgrad_plan(1, 1024, 1024, 8, 8, 3, has_bias=True, scratch_floats=9438208)[0]['accum'] == SLAB
    # a shape the tree does launch: the bbox head's first FC, 12544 -> 1024 as a 1x1 GEMM over 32 RoIs of one pixel
    # (bbox_heads.py: params_grad).  MT 8; J 12544: TN 128 costs 15680, TN 64 18816 -> JT 98: 784 tiles, one chunk, no split; the slab
    # would be 1024 x 12544 + 1024 floats
    one, = ops.conv2d_wgrad_plan(32, 1024, 12544, 1, 1, 1, has_bias=True)
    _is(one, gemm(1, 2, 2, 1), grid=784, MT=8, JT=98, splits=1, per_split=1, slabs=0, accum=ATOMICS)
    assert 1024 * 12544 + 1024 > BOUND


ERRORS = [
    ('Cout = 0', dict(cout=0)),
    ('Cs = 0', dict(cs=0)),
    ('NB = 0', dict(NB=0)),
    ('NB < 0', dict(NB=-1)),
    ('H = 0', dict(H=0)),
    ('W = 0', dict(W=0)),
    ('ksize = 2', dict(ks=2)),
    ('ksize = 5', dict(ks=5)),
    ('2^31 pixels', dict(NB=1 << 20, H=64, W=32)),
    ('no such mode', dict(mode=3)),
    ('negative mode', dict(mode=-1)),
    ('slab without scratch', dict(mode=SLAB, ws=0)),
    ('slab with negative scratch', dict(mode=SLAB, ws=-1)),
    ('one record of room', dict(cap=1)),
    ('null record array', dict(null=True)),
]


@pytest.mark.parametrize('name,change', ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_return_their_code_and_write_nothing(name, change):
    base = dict(cout=256, cs=256, NB=256, H=14, W=14, ks=3, bias=1, mode=SLAB, ws=BIG, io8=1, s16=1)

    def args(c):
        return (c['cout'] * c['H'] * c['W'], c['cout'], c['cs'] * c['H'] * c['W'], c['cs'], c['NB'], c['H'], c['W'], c['ks'], c['bias'],
                c['mode'], c['ws'], c['io8'], c['s16'])
    ok, rec = _raw(args(base), fill=-77)
    assert ok == 2 and -77 not in rec
    one, rec = _raw(args(dict(base, mode=FX)), fill=-77)
    assert one == 1 and rec[N_INTS:] == [-77] * N_INTS and -77 not in rec[:N_INTS]
    call = dict(base, **change)
    rc, rec = _raw(args(call), cap=call.get('cap', N_REC), null=call.get('null', False), fill=-77)
    assert rc == INVALID, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'
    with pytest.raises(RuntimeError, match='dm_conv2d_wgrad_plan'):
        ops.conv2d_wgrad_plan(0, 256, 256, 14, 14, 3)
