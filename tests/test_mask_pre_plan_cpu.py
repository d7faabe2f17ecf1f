"""dm_mask_pre_plan: the routes of the three launchers of csrc/mask_pre.hip (dm_bn_stats, dm_bn_relu_maxpool_fwd,
dm_bn_relu_maxpool_bwd), checked on numbers alone.  The plan takes the compute-unit count as an argument, so nothing here
depends on the device: every check runs at 256 units (the MI355X) and at two other counts.  `_model` restates the routing
rules from the header's description, independently of the C++; a sweep that crosses every threshold compares the two record
for record, and the boundaries that matter most are pinned by hand below it.  No GPU needed
(tests/test_mask_pre_gpu.py runs a case on every build named here)."""
import ctypes
import itertools

import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_MASK_PRE_PLAN_INTS'], CONSTS['DM_MASK_PRE_PLAN_MAX_LAUNCHES']
INVALID = CONSTS['DM_ERR_INVALID_ARG']
CUS = (256, 304, 64)
SPLITS, LDS_LIMIT = 16, 64 * 1024


def _raw(op, NB, C, H, W, scratch=1, align=16, cus=256, cap=N_REC, null=False, fill=-1):
    """dm_mask_pre_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([fill] * (N_INTS * N_REC)))
    rc = _lib.lib().dm_mask_pre_plan(int(op), NB, C, H, W, scratch, align, cus, None if null else rec, cap)
    return rc, list(rec)


def _launches(op, NB, C, H, W, **kw):
    """[(kernel name, P0, P1, P2, grid x, grid y, threads, LDS bytes, clear)] or the error code"""
    rc, rec = _raw(ops.MASK_PRE_OPS.index(op), NB, C, H, W, **kw)
    if rc < 0:
        return rc
    assert rec[rc * N_INTS:] == [-1] * ((N_REC - rc) * N_INTS)
    return [(ops.MASK_PRE_KERNELS[rec[i * N_INTS]],) + tuple(rec[i * N_INTS + 1:(i + 1) * N_INTS]) for i in range(rc)]


def _model(op, NB, C, H, W, scratch=1, align=16, cus=256):
    """The routes as include/dynamask_hip.h and the kernels' comments describe them."""
    HW, OHW = H * W, ((H - 1) // 2 + 1) * ((W - 1) // 2 + 1)
    if C <= 0 or H <= 0 or W <= 0 or NB < 0 or (NB == 0 and op != 'fwd'):
        return INVALID
    split = bool(scratch) and NB >= SPLITS
    if op == 'stats':
        if not split:
            return [('stats', 0, 0, 0, C, 1, 1024, 64, 0)]
        vec = int(HW % 4 == 0 and align >= 16)
        return [('stats_split', p, vec, 0, C, SPLITS, 256, 16, 0) for p in (0, 1)] + [('stats_finalize', 0, 0, 0, -(-C // 128), 1, 128, 0, 0)]
    if op == 'fwd':
        if NB == 0:
            return []
        pblocks = -(-OHW // 1024)
        if W % 2 == 0 and W >= 4 and OHW < 65536 and align >= 8:
            return [('fwd_rows', 0, 0, 0, NB * C * pblocks, 1, 256, 0, 0)]
        return [('fwd', 0, 0, 0, min(-(-NB * C * OHW // 256), 16384), 1, 256, 0, 0)]
    plane = 4 * (HW + 2 * OHW)
    quads = HW % 4 == 0 and align >= 16
    last = ('bn_bwd_split', 1, 0, 0, C, SPLITS, 256, 0, 0)
    if split and C * SPLITS >= 4 * cus and quads and plane + 16 <= LDS_LIMIT:
        even = int(H % 2 == 0 and W % 2 == 0 and W >= 4)
        pre = int(HW // 4 <= 1024 and OHW <= 1024)
        return [('pool_sums', even, pre, 0, C, SPLITS, 256, plane + 16, 0), last]
    if quads and plane <= LDS_LIMIT:
        pool = ('pool_lds', 0, 0, 0, min(NB * C, 16 * cus), 1, 256, plane, 0)
    else:
        pool = ('pool_scatter', 0, 0, 0, min(-(-NB * C * OHW // 256), 16384), 1, 256, 0, 1)
    return [pool, ('bn_bwd_split', 0, 0, 0, C, SPLITS, 256, 16, 0), last] if split else [pool, ('bn_bwd', 0, 0, 0, C, 1, 1024, 64, 0)]


MAPS = [(1, 1), (2, 2), (2, 3), (6, 2), (2, 6), (7, 9), (7, 12), (10, 6), (12, 20), (28, 28), (56, 56), (64, 64), (66, 64), (65, 68),
        (112, 112), (1, 8188), (1, 8192), (1, 8196), (510, 512), (512, 512)]
BATCHES = (0, 1, 15, 16, 17)
CHANNELS = (1, 3, 15, 16, 17, 63, 64, 65, 75, 76, 77, 300)      # cus / 4 = 64, 76, 16: the sums route's threshold and its neighbours


def test_record_layout_and_names():
    assert N_INTS == len(ops.MASK_PRE_PLAN_FIELDS) == 9 and N_REC == 3
    assert [CONSTS['DM_MASK_PRE_' + n.upper()] for n in ops.MASK_PRE_OPS] == [0, 1, 2] and set(ops.MASK_PRE_BUILDS) == set(ops.MASK_PRE_OPS)
    named = [b[0] for builds in ops.MASK_PRE_BUILDS.values() for b in builds]
    assert len(ops.MASK_PRE_KERNELS) == 10 == len(set(named)) and sorted(set(named)) == list(range(10))
    assert sum(len(b) for b in ops.MASK_PRE_BUILDS.values()) == 6 + 2 + 9


@pytest.mark.parametrize('cus', CUS)
def test_the_plan_is_the_model_on_a_sweep_across_every_threshold_and_names_every_build(cus):
    reached = {op: set() for op in ops.MASK_PRE_OPS}
    bad, n = [], 0
    for op, NB, C, (H, W), scratch, align in itertools.product(ops.MASK_PRE_OPS, BATCHES, CHANNELS, MAPS, (0, 1), (4, 8, 16)):
        got, want = _launches(op, NB, C, H, W, scratch=scratch, align=align, cus=cus), _model(op, NB, C, H, W, scratch, align, cus)
        n += 1
        if got != want:
            bad.append(((op, NB, C, H, W, scratch, align), got, want))
            continue
        if got == INVALID:
            continue
        builds = {(ops.MASK_PRE_KERNELS.index(l[0]),) + l[1:4] for l in got}
        assert builds <= ops.MASK_PRE_BUILDS[op], (op, NB, C, H, W, scratch, align)
        reached[op] |= builds
        # the alignment a kernel's widest access needs, the scratch the split kernels write, LDS within the limit
        for k, p0, p1, _, gx, gy, threads, lds, clear in got:
            assert align >= 16 or (k not in ('pool_lds', 'pool_sums') and not (k == 'stats_split' and p1)), (op, NB, C, H, W, align, k)
            assert align >= 8 or k != 'fwd_rows'
            assert scratch or k not in ('stats_split', 'stats_finalize', 'pool_sums', 'bn_bwd_split')
            assert 0 <= lds <= LDS_LIMIT and gx >= 1 and gy >= 1 and clear == (k == 'pool_scatter')
    assert not bad, (len(bad), bad[:3])
    assert n > 20000 and reached == ops.MASK_PRE_BUILDS


@pytest.mark.parametrize('cus', CUS)
def test_the_sums_route_starts_at_four_workgroups_per_compute_unit(cus):
    """C * 16 >= 4 * CUs: the channel count the GPU cases look for (64 at 256 units)."""
    c = cus // 4
    first = [_launches('bwd', 16, ch, 12, 20, cus=cus)[0][0] for ch in (c - 1, c, c + 1)]
    assert first == ['pool_lds', 'pool_sums', 'pool_sums']
    assert [l[0] for l in _launches('bwd', 16, c - 1, 12, 20, cus=cus)] == ['pool_lds', 'bn_bwd_split', 'bn_bwd_split']
    assert [l[:3] for l in _launches('bwd', 16, c, 12, 20, cus=cus)] == [('pool_sums', 1, 1), ('bn_bwd_split', 1, 0)]
    # fifteen images, or no scratch: no split form at all, however many channels
    for kw in (dict(NB=15), dict(NB=16, scratch=0)):
        assert [l[0] for l in _launches('bwd', kw.pop('NB'), 4 * c, 12, 20, cus=cus, **kw)] == ['pool_lds', 'bn_bwd']
    # the plane kernel's workgroups walk several planes from 16 per unit on
    assert _launches('bwd', 15, 300, 2, 2, cus=cus)[0][4] == min(4500, 16 * cus)


@pytest.mark.parametrize('cus', CUS)
def test_the_forms_of_the_sums_kernel(cus):
    c = cus // 4
    form = lambda H, W: _launches('bwd', 16, c, H, W, cus=cus)[0][:3]      # noqa: E731
    # prefetch: a plane's quads and its pooled gradients fit four slots of 256 threads -- 64 x 64 fills every slot
    assert form(64, 64) == ('pool_sums', 1, 1) and form(66, 64) == ('pool_sums', 1, 0)
    assert form(56, 56) == ('pool_sums', 1, 1) and form(28, 28) == ('pool_sums', 1, 1)
    assert form(7, 12) == ('pool_sums', 0, 1) and form(65, 68) == ('pool_sums', 0, 0)
    # 2 x 2 blocks need H and W even and W >= 4
    assert form(2, 6) == ('pool_sums', 1, 1) and form(6, 2) == ('pool_sums', 0, 1) and form(3, 4) == ('pool_sums', 0, 1)
    assert form(7, 9)[0] == 'pool_scatter'           # H * W % 4 != 0


@pytest.mark.parametrize('cus', CUS)
def test_lds_is_counted_static_plus_dynamic(cus):
    c = cus // 4
    # 1 x 8192: 8192 + 2 x 4096 floats = 64 KB of plane.  The sums kernel's 16 static bytes do not fit beside it; the plane kernel
    # has none.  Four columns fewer and the sums kernel fits, with its 16 bytes in the record; four more and neither does
    assert _launches('bwd', 16, c, 1, 8192, cus=cus) == _model('bwd', 16, c, 1, 8192, cus=cus)
    assert [l[0] for l in _launches('bwd', 16, c, 1, 8192, cus=cus)] == ['pool_lds', 'bn_bwd_split', 'bn_bwd_split']
    assert _launches('bwd', 16, c, 1, 8192, cus=cus)[0][7] == LDS_LIMIT
    assert _launches('bwd', 16, c, 1, 8188, cus=cus)[0][:3] + _launches('bwd', 16, c, 1, 8188, cus=cus)[0][7:] == ('pool_sums', 0, 0, 65520, 0)
    assert _launches('bwd', 16, c, 1, 8196, cus=cus)[0][0] == 'pool_scatter'
    assert _launches('bwd', 1, 2, 112, 112, cus=cus)[0] == ('pool_scatter', 0, 0, 0, 25, 1, 256, 0, 1)      # 2 x 56 x 56 outputs in 256s
    assert _launches('bwd', 16, c, 56, 56, cus=cus)[0][7] == 4 * (3136 + 2 * 784) + 16


def test_alignment_and_scratch_facts():
    # the backward's plane kernels and the vector loop of the split statistics: 16 bytes; the rows forward: 8
    first = lambda op, shape, **kw: _launches(op, *shape, **kw)[0][:3]      # noqa: E731
    assert [first('bwd', (16, 64, 12, 20), align=a) for a in (16, 8, 4)] == [('pool_sums', 1, 1), ('pool_scatter', 0, 0), ('pool_scatter', 0, 0)]
    assert [first('bwd', (3, 5, 10, 6), align=a) for a in (16, 8, 4)] == [('pool_lds', 0, 0), ('pool_scatter', 0, 0), ('pool_scatter', 0, 0)]
    assert [first('fwd', (2, 3, 12, 20), align=a) for a in (16, 8, 4)] == [('fwd_rows', 0, 0), ('fwd_rows', 0, 0), ('fwd', 0, 0)]
    assert [first('stats', (16, 6, 7, 8), align=a) for a in (16, 8, 4)] == [('stats_split', 0, 1), ('stats_split', 0, 0), ('stats_split', 0, 0)]
    assert first('stats', (16, 6, 7, 9)) == ('stats_split', 0, 0)            # H * W % 4 != 0: the scalar loop
    # the scratch
    assert [l[0] for l in _launches('stats', 16, 6, 7, 8, scratch=0)] == ['stats'] == [l[0] for l in _launches('stats', 15, 6, 7, 8)]
    assert [l[0] for l in _launches('bwd', 16, 64, 12, 20, scratch=0)] == ['pool_lds', 'bn_bwd']
    assert _launches('fwd', 2, 3, 12, 20, scratch=0) == _launches('fwd', 2, 3, 12, 20, scratch=1)
    # the forward's other conditions: odd W, W = 2, 65536 outputs a plane; two blocks a plane from 1025 outputs on
    assert first('fwd', (2, 7, 7, 9))[0] == 'fwd' == first('fwd', (2, 3, 6, 2))[0] == first('fwd', (1, 1, 512, 512))[0]
    assert _launches('fwd', 1, 2, 66, 64)[0][:5] == ('fwd_rows', 0, 0, 0, 4) and _launches('fwd', 1, 2, 64, 64)[0][4] == 2
    assert _launches('fwd', 1, 1, 510, 512)[0][:5] == ('fwd_rows', 0, 0, 0, 64)


def test_hand_derived_pins_of_the_training_shapes():
    # MaskPre at 256 RoIs and 256 units: 128 channels at 56 x 56 (128 x 16 >= 1024: the sums kernel, blocks, prefetch; 12544 +
    # 2 x 3136 bytes of plane + 16), 16 channels at 28 x 28 (256 < 1024: the plane kernel, one workgroup a plane up to 4096)
    plan = lambda *a, **kw: ops.mask_pre_plan(*a, cus=256, **kw)      # noqa: E731
    assert plan('bwd', 256, 128, 56, 56) == [
        dict(kernel=7, P0=1, P1=1, P2=0, grid_x=128, grid_y=16, threads=256, lds_bytes=18832, clear=0),
        dict(kernel=9, P0=1, P1=0, P2=0, grid_x=128, grid_y=16, threads=256, lds_bytes=0, clear=0)]
    assert plan('bwd', 256, 16, 28, 28) == [
        dict(kernel=6, P0=0, P1=0, P2=0, grid_x=4096, grid_y=1, threads=256, lds_bytes=4704, clear=0),
        dict(kernel=9, P0=0, P1=0, P2=0, grid_x=16, grid_y=16, threads=256, lds_bytes=16, clear=0),
        dict(kernel=9, P0=1, P1=0, P2=0, grid_x=16, grid_y=16, threads=256, lds_bytes=0, clear=0)]
    assert plan('fwd', 256, 128, 56, 56) == [dict(kernel=4, P0=0, P1=0, P2=0, grid_x=32768, grid_y=1, threads=256, lds_bytes=0, clear=0)]
    assert [r['kernel'] for r in plan('stats', 256, 128, 56, 56)] == [1, 1, 2] and plan('stats', 256, 128, 56, 56)[2]['grid_x'] == 1
    assert plan('stats', 4, 129, 7, 8, scratch=False) == [dict(kernel=0, P0=0, P1=0, P2=0, grid_x=129, grid_y=1, threads=1024, lds_bytes=64, clear=0)]
    # aligned: True / False or the bytes
    assert plan('bwd', 16, 64, 12, 20, aligned=False) == plan('bwd', 16, 64, 12, 20, aligned=4) == plan('bwd', 16, 64, 12, 20, aligned=8)
    assert plan('bwd', 16, 64, 12, 20, aligned=True) == plan('bwd', 16, 64, 12, 20, aligned=16) != plan('bwd', 16, 64, 12, 20, aligned=8)
    assert plan('fwd', 0, 3, 12, 20) == []
    # without a count the device's is taken, 256 where there is none
    assert ops.mask_pre_plan('fwd', 2, 3, 12, 20) == plan('fwd', 2, 3, 12, 20)
    with pytest.raises(RuntimeError, match='dm_mask_pre_plan'):
        ops.mask_pre_plan('bwd', 0, 3, 12, 20)


ERRORS = [
    ('no such op', dict(op=3)),
    ('negative op', dict(op=-1)),
    ('no images', dict(NB=0)),
    ('negative images', dict(NB=-1)),
    ('no channels', dict(C=0)),
    ('no rows', dict(H=0)),
    ('no columns', dict(W=-3)),
    ('a plane beyond 2^31 elements', dict(H=1 << 16, W=1 << 16)),
    ('an alignment that is none', dict(align=12)),
    ('two records of room', dict(cap=2)),
    ('null record array', dict(null=True)),
]


@pytest.mark.parametrize('name,change', ERRORS, ids=[e[0] for e in ERRORS])
@pytest.mark.parametrize('op', (0, 2), ids=('stats', 'bwd'))
def test_error_paths_return_their_code_and_write_nothing(op, name, change):
    base = dict(op=op, NB=16, C=64, H=12, W=20)
    ok, rec = _raw(**base, fill=-77)
    assert ok in (2, 3) and -77 not in rec[:ok * N_INTS] and rec[ok * N_INTS:] == [-77] * ((N_REC - ok) * N_INTS)
    rc, rec = _raw(**dict(base, **change), fill=-77)
    assert rc == INVALID, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'


def test_the_forward_refuses_like_its_launcher_and_takes_an_empty_call():
    for change in (dict(NB=-1), dict(C=0), dict(H=0), dict(W=0), dict(align=0)):
        rc, rec = _raw(**dict(dict(op=1, NB=2, C=3, H=12, W=20), **change), fill=-77)
        assert rc == INVALID and rec == [-77] * (N_INTS * N_REC)
    rc, rec = _raw(1, 0, 3, 12, 20, fill=-77)
    assert rc == 0 and rec == [-77] * (N_INTS * N_REC)
