"""dm_bwd_plan: the routes of the six training-side launchers of csrc/backward.hip (dm_deform_im2col, dm_deform_coord_grad,
dm_deform_col2im, dm_upsample2x_bilinear_bwd, dm_point_sample_bwd[_fx], dm_class_logits_bwd[_slab, _fx]), pinned at the
256-CU fallback of a machine without a device.  tests/golden/bwd_plan_256cu.npz is the routing of those launchers as it was
BEFORE they were restructured into validate / route / emit: recorded from that code with a recorder at each of its twenty
launch sites, over a grid that crosses every threshold (tools/bwd_plan_table.py regenerates it from the current library; a
routing change is meant to show up as a diff of that table).  No GPU needed; on a machine WITH a device the compute-unit
count is the device's and the replay is skipped where it differs (tests/test_bwd_builds_gpu.py asks the plan there)."""
import ctypes
import os

import numpy as np
import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_BWD_PLAN_INTS'], CONSTS['DM_BWD_PLAN_MAX_LAUNCHES']
INVALID, UNSUPPORTED = CONSTS['DM_ERR_INVALID_ARG'], CONSTS['DM_ERR_UNSUPPORTED']
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'bwd_plan_256cu.npz')
COUNTS = (5, 5, 5, 4, 7, 7)
IM2COL, COORD_GRAD, COL2IM, UPSAMPLE, POINT_SAMPLE, CLASS_LOGITS = range(6)
ATOMICS, SLAB, FX = range(3)
R_KERNEL, R_P0, R_P2, R_GX, R_GY, R_THREADS, R_LDS, R_CLEAR = 0, 1, 3, 4, 5, 6, 7, 8


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


needs_256 = pytest.mark.skipif(_cus() != 256, reason='recorded at the 256-CU count the library assumes without a device')


def _raw(op, numbers, count=None, cap=N_REC, null=False, fill=-1):
    """dm_bwd_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([fill] * (N_INTS * N_REC)))
    nums = (ctypes.c_longlong * max(1, len(numbers)))(*[int(v) for v in numbers])
    rc = _lib.lib().dm_bwd_plan(int(op), nums, len(numbers) if count is None else count, None if null else rec, cap)
    return rc, list(rec)


def test_record_layout_and_names():
    assert N_INTS == len(ops.BWD_PLAN_FIELDS) == 9 and N_REC == 2
    assert [CONSTS['DM_BWD_' + n.upper()] for n in ops.BWD_OPS] == list(range(6)) == sorted(ops.BWD_OPS.index(o) for o in ops.BWD_BUILDS)
    assert len(ops.BWD_KERNELS) == 14 == len({b[0] for builds in ops.BWD_BUILDS.values() for b in builds})
    assert os.path.getsize(TABLE) < 1 << 20


@needs_256
def test_the_library_reproduces_the_recorded_table_row_for_row():
    t = np.load(TABLE)
    op, args, rcs, recs = t['op'], t['args'], t['rc'], t['rec']
    assert len(op) == len(args) == len(rcs) == len(recs) > 20000 and recs.shape[1] == N_INTS * N_REC and args.shape[1] == 7
    bad = []
    for o, a, rc, rec in zip(op.tolist(), args.tolist(), rcs.tolist(), recs.tolist()):
        got = _raw(o, a[:COUNTS[o]])
        if got != (rc, rec):
            bad.append((o, a, (rc, rec), got))
    assert not bad, (len(bad), bad[:3])


def test_the_table_names_every_kernel_and_build_and_no_other():
    """(kernel, build) values do not depend on the compute-unit count: no skip."""
    t = np.load(TABLE)
    op, rcs, recs = t['op'], t['rc'], t['rec']
    for i, name in enumerate(ops.BWD_OPS):
        mine = recs[(op == i) & (rcs >= 1)]
        named = {tuple(r[:4]) for r in mine[:, :N_INTS].tolist()} | {tuple(r[:4]) for r in mine[mine[:, N_INTS] >= 0][:, N_INTS:].tolist()}
        assert named == ops.BWD_BUILDS[name], name


def test_the_table_covers_the_routes():
    t = np.load(TABLE)
    op, args, rcs, recs = t['op'], t['args'], t['rc'], t['rec']
    first = recs[:, :N_INTS]
    # every return code of every launcher: refused as invalid, an empty call, one launch; unsupported and two launches where
    # the launcher has them; nothing written on a refusal, one record for one launch
    want = {IM2COL: {INVALID, UNSUPPORTED, 0, 1}, COORD_GRAD: {INVALID, 0, 1}, COL2IM: {INVALID, UNSUPPORTED, 0, 1},
            UPSAMPLE: {INVALID, 0, 1}, POINT_SAMPLE: {INVALID, 0, 1}, CLASS_LOGITS: {INVALID, 0, 1, 2}}
    for o, codes in want.items():
        assert set(rcs[op == o].tolist()) == codes, o
    assert (recs[rcs <= 0] == -1).all() and (recs[rcs == 1][:, N_INTS:] == -1).all() and (recs[rcs == 2] >= 0).all()
    # im2col refuses W < 2 before it returns from an empty call, and an invalid argument before either
    im = op == IM2COL
    assert (rcs[im & (args[:, 3] == 1) & (args[:, 0] == 0) & (args[:, 1] > 0)] == UNSUPPORTED).all()
    assert (rcs[im & (args[:, 3] == 1) & (args[:, 1] <= 0)] == INVALID).all()
    # col2im returns from an empty call before it refuses a plane that does not fit
    c2 = (op == COL2IM) & (args[:, 2] * args[:, 3] > 8192)
    assert set(rcs[c2 & (args[:, 0] > 0)].tolist()) == {UNSUPPORTED} and set(rcs[c2 & (args[:, 0] == 0)].tolist()) == {0}
    # only the upsample scatter clears its output; only the class-logit slab form has a second launch, always the reduce
    assert ((first[:, R_CLEAR] == 1) == ((rcs == 1) & (first[:, R_KERNEL] == ops.BWD_KERNELS.index('upsample_scatter')))).all()
    cl = op == CLASS_LOGITS
    assert ((rcs == 2) == (cl & (rcs >= 1) & (args[:, 4] == SLAB))).all()
    assert set(recs[rcs == 2][:, N_INTS + R_KERNEL].tolist()) == {ops.BWD_KERNELS.index('class_logits_reduce')}
    # the accumulation taken is the one asked for
    ok = cl & (rcs >= 1)
    assert (first[ok][:, R_P2] == args[ok][:, 4]).all()
    ps = (op == POINT_SAMPLE) & (rcs == 1)
    assert (first[ps][:, R_P2] == 2 * args[ps][:, 6]).all()
    # a misaligned class-logit call never takes the wave kernel; an aligned one does for HW % 4 == 0 up to 1024
    wave = first[:, R_KERNEL] == ops.BWD_KERNELS.index('class_logits_wave')
    assert not wave[ok & (args[:, 5] == 0)].any()
    assert (wave[ok & (args[:, 5] == 1)] == ((args[ok & (args[:, 5] == 1)][:, 2] % 4 == 0) & (args[ok & (args[:, 5] == 1)][:, 2] <= 1024))).all()
    # a slab call is refused one float short of dm_class_logits_bwd_scratch_floats and beyond 65535 classes
    slab = cl & (args[:, 4] == SLAB) & (args[:, 0] >= 0) & (args[:, 1] > 0) & (args[:, 2] > 0) & (args[:, 3] > 0)
    need = 2 * args[:, 0] * args[:, 1] + 2 * args[:, 0]
    assert ((rcs[slab] == INVALID) == ((args[slab][:, 6] < need[slab]) | (args[slab][:, 3] > 65535))).all()
    assert (args[slab][:, 6] == need[slab] - 1).sum() > 100 and (args[slab][:, 3] == 65536).sum() > 100


@needs_256
def test_hand_derived_pins():
    # the training shapes.  DCN at 14 x 14, 256 channels, one group, 256 RoIs: im2col CT 32 (196 px x 32 planes x 4 B = 25088 B),
    # 256 x 8 workgroups; the coordinate gradient: one band of 14 rows, slots 2 x 16 x 16 = 512 -> <4, 2, 512>, 16 KB; col2im CT 8:
    # 8 x 196 x 8 B = 12544 B, 256 x 32 workgroups
    one, = ops.backward_plan('im2col', 256, 256, 14, 14, 1)
    assert one == dict(kernel=0, P0=32, P1=0, P2=0, grid_x=2048, grid_y=1, threads=256, lds_bytes=25088, clear=0)
    one, = ops.backward_plan('coord_grad', 256, 256, 14, 14, 1)
    assert one == dict(kernel=2, P0=4, P1=2, P2=512, grid_x=256, grid_y=1, threads=512, lds_bytes=16384, clear=0)
    one, = ops.backward_plan('col2im', 256, 256, 14, 14, 1)
    assert one == dict(kernel=4, P0=8, P1=0, P2=0, grid_x=8192, grid_y=1, threads=256, lds_bytes=12544, clear=0)
    # 56 x 56, 64 channels: two planes of 25088 B in 512 threads; the coordinate gradient in 14 bands of 4 rows, 14 staged:
    # slots 2 x 16 x 58 = 1856 -> <2, 2, 1024>
    one, = ops.backward_plan('col2im', 256, 64, 56, 56, 1)
    assert (one['P0'], one['threads'], one['lds_bytes'], one['grid_x']) == (2, 512, 50176, 256 * 32)
    one, = ops.backward_plan('coord_grad', 256, 64, 56, 56, 1)
    assert (one['P0'], one['P1'], one['P2'], one['grid_x'], one['lds_bytes']) == (2, 2, 1024, 256 * 14, 1856 * 32)
    # the logit gradients, 256 planes of 112 x 112 from 56 x 56, align_corners: 256 <= 512 -> 1024 threads, 24 x 3136 B
    one, = ops.backward_plan('upsample', 256, 56, 56, align_corners=True)
    assert one == dict(kernel=7, P0=1024, P1=0, P2=0, grid_x=256, grid_y=1, threads=1024, lds_bytes=75264, clear=0)
    one, = ops.backward_plan('upsample', 513, 56, 56, align_corners=True)
    assert (one['P0'], one['threads'], one['grid_x']) == (256, 256, 513)
    one, = ops.backward_plan('upsample', 5000, 14, 14)
    assert (one['kernel'], one['grid_x'], one['lds_bytes']) == (5, 2048, 16 * 196)
    one, = ops.backward_plan('upsample', 3, 72, 72, align_corners=True)          # 24 x 5184 B > 96 KB: cleared, scattered
    assert (one['kernel'], one['clear'], one['grid_x']) == (8, 1, 3 * 4 * 5184 // 256)
    # the class logits at 28 x 28 (HW 784 > 256: four quads a lane), 7 RoIs of 64 channels, 80 classes: 4 x 7 workgroups, then
    # the reduce over 64 / 16 channel groups x 80 classes
    first, red = ops.backward_plan('class_logits', 7, 64, 784, 80, mode='slab')
    assert first == dict(kernel=11, P0=4, P1=4, P2=SLAB, grid_x=4, grid_y=7, threads=256, lds_bytes=0, clear=0)
    assert red == dict(kernel=13, P0=0, P1=0, P2=SLAB, grid_x=4, grid_y=80, threads=256, lds_bytes=0, clear=0)
    one, = ops.backward_plan('class_logits', 7, 64, 784, 80, mode='fx', aligned16=False)
    assert (one['kernel'], one['P2'], one['grid_x'], one['grid_y']) == (12, FX, 64, 7)
    # the point sample at 14 samples: 4 (4 x 196 + 56 + 3 x 46 + 3 x 29) = 4260 B of tables
    one, = ops.backward_plan('point_sample', 2, 22, 25, 42, 11, 14, mode='atomics')
    assert one == dict(kernel=9, P0=4, P1=0, P2=ATOMICS, grid_x=6, grid_y=11, threads=256, lds_bytes=4260, clear=0)
    one, = ops.backward_plan('point_sample', 2, 22, 25, 42, 11, 64, mode='fx')
    assert (one['kernel'], one['P2'], one['lds_bytes']) == (10, FX, 49152)


def test_backward_plan_follows_the_module_flags():
    saved = ops.CLB_SLAB[0], ops.DETERMINISTIC[0]
    try:
        for slab, det, mode, launches in ((True, False, SLAB, 2), (True, True, SLAB, 2), (False, True, FX, 1), (False, False, ATOMICS, 1)):
            ops.CLB_SLAB[0], ops.DETERMINISTIC[0] = slab, det
            recs = ops.backward_plan('class_logits', 7, 64, 196, 80)
            assert len(recs) == launches and recs[0]['P2'] == mode
            assert ops.backward_plan('point_sample', 2, 8, 25, 42, 3, 14)[0]['P2'] == (FX if det else ATOMICS)
        assert ops.backward_plan('class_logits', 0, 64, 196, 80) == [] == ops.backward_plan('col2im', 0, 64, 14, 14, 1)
    finally:
        ops.CLB_SLAB[0], ops.DETERMINISTIC[0] = saved
    with pytest.raises(RuntimeError, match='dm_bwd_plan'):
        ops.backward_plan('col2im', 1, 8, 100, 100, 1)
    with pytest.raises(RuntimeError, match='dm_bwd_plan'):
        ops.backward_plan('im2col', 1, 8, 14, 1, 1)


ERRORS = [
    ('no such op', dict(op=6)),
    ('negative op', dict(op=-1)),
    ('a number short', dict(count=4)),
    ('a number more', dict(numbers=(2, 16, 14, 14, 2, 0), count=6)),
    ('a number that is no int', dict(numbers=(2, 16, 14, 1 << 31, 2))),
    ('invalid argument', dict(numbers=(2, 16, 14, 14, 3))),
    ('one record of room', dict(cap=1)),
    ('null record array', dict(null=True)),
]


@pytest.mark.parametrize('name,change', ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_return_their_code_and_write_nothing(name, change):
    base = dict(op=COL2IM, numbers=(2, 16, 14, 14, 2), count=None, cap=N_REC, null=False)
    ok, rec = _raw(**base, fill=-77)
    assert ok == 1 and rec[N_INTS:] == [-77] * N_INTS and -77 not in rec[:N_INTS]
    two, rec = _raw(CLASS_LOGITS, (7, 64, 196, 80, SLAB, 1, 1 << 40), fill=-77)
    assert two == 2 and -77 not in rec
    rc, rec = _raw(**dict(base, **change), fill=-77)
    assert rc == INVALID, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'
    rc, rec = _raw(COL2IM, (2, 16, 100, 100, 2), fill=-77)
    assert rc == UNSUPPORTED and rec == [-77] * (N_INTS * N_REC)
