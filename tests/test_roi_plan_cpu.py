"""dm_roi_align_plan: the RoIAlign launchers' own route (csrc/roi_align.hip: roi_route, the value roi_emit enqueues).
tests/golden/roi_plan.npz is the routing of the launchers as they were BEFORE they were restructured into validate / route /
emit: recorded from that code with a recorder at each of its launch sites and error returns, over a grid that crosses every
threshold (tools/roi_plan_table.py has the grid and regenerates the table from the current library; a routing change is meant
to show up as a diff of that table).  Two fields of a record say what no kernel reads and were set by the recording, not by
the old launchers: the order kernel's CT / order / lds_floats (0) and the gather backward's CT (4, its one channel quad).
The hand-derived pins below carry their arithmetic in the comment next to them.  No GPU needed, and none changes the answer:
nothing in this route reads the compute-unit count."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_ROI_PLAN_INTS'], CONSTS['DM_ROI_PLAN_MAX_LAUNCHES']
INVALID, UNSUPPORTED = CONSTS['DM_ERR_INVALID_ARG'], CONSTS['DM_ERR_UNSUPPORTED']
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'roi_plan.npz')
KNOBS = ({}, {'DM_ROI_SORT': '0'}, {'DM_ROI_SORT_MIN': '1'})              # column 20 of a row: the environment it is planned under
FWD, ADD, BWD = range(3)
ORDER, TILE, BAND, GENERIC, GATHER = range(5)
PYRAMID = [(200, 336), (100, 168), (50, 84), (25, 42)]                   # the FPN maps of a 1333 x 800 image
TILE_LDS = (2048 + 64) * 16                                              # the staging buffer + the stencil table, float4 words


@contextlib.contextmanager
def knobs(k):
    names = ('DM_ROI_SORT', 'DM_ROI_SORT_MIN')
    was = {n: os.environ.get(n) for n in names}
    try:
        for n in names:
            os.environ.pop(n, None)
        os.environ.update(KNOBS[k])
        _lib.lib().dm_reload_env_knobs()
        yield
    finally:
        for n in names:
            os.environ.pop(n, None)
            if was[n] is not None:
                os.environ[n] = was[n]
        _lib.lib().dm_reload_env_knobs()


def _raw(a, cap=N_REC, null=False, fill=-1):
    """One table row (its first 20 columns) straight through ctypes, the record array filled with a canary."""
    a = [int(v) for v in a]
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([fill] * (N_INTS * N_REC)))
    rc = _lib.lib().dm_roi_align_plan(a[0], a[1], a[2], (ctypes.c_int * 5)(*a[3:8]), (ctypes.c_int * 5)(*a[8:13]), *a[13:20],
                                      None if null else rec, cap)
    return rc, list(rec)


def _is(rec, **want):
    got = {k: rec[k] for k in want}
    assert got == want, (got, want)


@pytest.fixture(scope='module')
def table():
    t = np.load(TABLE)
    return t['args'], t['rc'], t['rec']


def test_record_layout_and_field_names():
    assert N_INTS == len(ops.ROI_PLAN_FIELDS) == 10 and N_REC == 2
    assert ops.ROI_KERNELS == ('order', 'tile', 'band', 'generic', 'bwd_gather') and ops.ROI_ENTRIES == ('forward', 'add', 'backward')
    assert ops.roi_align_plan('forward', PYRAMID, 2, 256, 0, 14) == []    # N = 0: DM_OK, nothing launched
    assert os.path.getsize(TABLE) < 1 << 20


def test_the_library_reproduces_the_recorded_table_row_for_row(table):
    args, rcs, recs = table
    assert len(args) == len(rcs) == len(recs) > 40000 and recs.shape[1] == N_INTS * N_REC and args.shape[1] == 21
    bad = []
    for k in range(len(KNOBS)):
        with knobs(k):
            for i in np.nonzero(args[:, 20] == k)[0].tolist():
                got = _raw(args[i, :20])
                if got != (int(rcs[i]), recs[i].tolist()):
                    bad.append((args[i].tolist(), (int(rcs[i]), recs[i].tolist()), got))
    assert not bad, (len(bad), bad[:3])
    # the table does cross the routes: every build of every entry, under every knob setting, and every return code
    assert set(rcs.tolist()) == {INVALID, UNSUPPORTED, 0, 1, 2}
    assert set(args[:, 20].tolist()) == {0, 1, 2}
    ok = rcs >= 1
    first, last = recs[ok][:, :3], np.where((rcs[ok] == 2)[:, None], recs[ok][:, N_INTS:N_INTS + 3], recs[ok][:, :3])
    builds = lambda entry, part: {tuple(r) for r in part[args[ok][:, 0] == entry].tolist()}      # noqa: E731
    assert builds(FWD, first) == {(ORDER, 0, 0), (TILE, 0, 0), (BAND, 2048, 4), (GENERIC, 0, 1)}
    assert builds(FWD, last) == {(TILE, 0, 0), (BAND, 2048, 4), (GENERIC, 0, 2)}
    assert builds(ADD, first) == {(TILE, 1, 0), (TILE, 2, 0)} and builds(BWD, first) == {(GENERIC, 1, 0), (GATHER, 0, 0)}
    fwd_tile = recs[ok & (args[:, 0] == FWD)]
    plain, ordered = fwd_tile[fwd_tile[:, 0] == TILE], fwd_tile[fwd_tile[:, 0] == ORDER]
    assert set(plain[:, 6].tolist()) == {16} and set(ordered[:, N_INTS + 6].tolist()) == {32}        # CT of the two tile routes
    assert set(plain[:, 7].tolist()) == set(ordered[:, N_INTS + 7].tolist()) == {0, 1}               # both workgroup orders
    # ordered rows exist under the default knobs and DM_ROI_SORT_MIN = 1, never with DM_ROI_SORT = 0
    assert {int(a[20]) for a in args[ok & (recs[:, 0] == ORDER)]} == {0, 2}
    # every error code for every entry; UNSUPPORTED for the forward and the backward: a grid beyond 2^31 only -- none here
    for entry, codes in ((FWD, {INVALID}), (ADD, {INVALID, UNSUPPORTED}), (BWD, {INVALID})):
        assert set(rcs[(args[:, 0] == entry) & (rcs < 0)].tolist()) == codes


def test_headline_512_rois_ordered_and_plain():
    # 512 RoIs x 256 channels, 14 x 14, the pyramid, the workspace the library asks for (512 x 32 bytes).  The order kernel
    # ranks 256 / 16 threads-per-RoI = 16 RoIs per workgroup: ceil(512 / 16) = 32 workgroups, no LDS beyond its static keys,
    # and writes the levels.  The tile kernel behind it: 32 channels per workgroup -> 256 / 32 = 8 chunks, 8 % 8 == 0 -> the
    # XCD-aware order, 512 x 8 = 4096 workgroups, (2048 + 64) float4 of LDS.
    assert _lib.lib().dm_roi_align_workspace_bytes(512, 14) == 512 * 32
    order, tile = ops.roi_align_plan('forward', PYRAMID, 2, 256, 512, 14)
    _is(order, kernel=ORDER, P0=0, P1=0, grid=32, threads=256, lds_bytes=0, CT=0, order=0, lds_floats=0, levels=1)
    _is(tile, kernel=TILE, P0=0, P1=0, grid=4096, threads=256, lds_bytes=TILE_LDS, CT=32, order=1, lds_floats=0, levels=0)
    # without a workspace: 16 channels per workgroup -> 16 chunks, 16 % 8 == 0 -> order 1, 512 x 16 = 8192; it writes the levels
    for ws in (0, 512 * 32 - 1):
        one, = ops.roi_align_plan('forward', PYRAMID, 2, 256, 512, 14, workspace=ws)
        _is(one, kernel=TILE, P0=0, P1=0, grid=8192, threads=256, lds_bytes=TILE_LDS, CT=16, order=1, lds_floats=0, levels=1)
    assert ops.roi_align_plan_raw('forward', PYRAMID, 2, 256, 512, 14, workspace_bytes=512 * 32, workspace=2)[1] == [one]   # misaligned
    # neither B nor the sampling ratio enters the route
    assert ops.roi_align_plan('forward', PYRAMID, 7, 256, 512, 14, sampling_ratio=2) == [order, tile]
    # 100 channels: 7 chunks of 16 (6.25), 7 % 8 != 0 -> launch order; ordered: 4 chunks of 32 (3.1) -> launch order too
    _is(ops.roi_align_plan('forward', PYRAMID, 2, 100, 512, 14, workspace=0)[0], CT=16, order=0, grid=512 * 7)
    _is(ops.roi_align_plan('forward', PYRAMID, 2, 100, 512, 14)[1], CT=32, order=0, grid=512 * 4)
    # 128 channels: 8 chunks of 16 -> order 1; ordered 4 chunks of 32 -> order 0
    _is(ops.roi_align_plan('forward', PYRAMID, 2, 128, 512, 14, workspace=0)[0], CT=16, order=1, grid=4096)
    _is(ops.roi_align_plan('forward', PYRAMID, 2, 128, 512, 14)[1], CT=32, order=0, grid=2048)


def test_ordering_thresholds_and_the_workspace_bound():
    wsb = _lib.lib().dm_roi_align_workspace_bytes
    # 192 .. 1024 RoIs; P x P in [128, 256]: P = 12 .. 16
    for N, P, want in ((191, 14, 0), (192, 14, 192 * 32), (1024, 14, 1024 * 32), (1025, 14, 0), (512, 11, 0), (512, 12, 512 * 32),
                       (512, 16, 512 * 32), (512, 17, 0), (512, 7, 0), (0, 14, 0), (-5, 14, 0), (512, -14, 0), (512, 1, 0)):
        assert wsb(N, P) == want, (N, P)
        if N > 0 and P > 0:
            got = [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 256, N, P)]
            assert (got == [ORDER, TILE]) == (want > 0), (N, P, got)
            # an upper bound the route honours: more changes nothing, one byte less orders nothing
            more = [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 256, N, P, workspace=N * 32 + 4096)]
            assert more == got, (N, P)
            if want:
                assert [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 256, N, P, workspace=want - 1)] == [TILE]
    # a call the bound says would order may still not: channels not in quads (the generic kernel), a map above 2^23 pixels
    assert [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 6, 512, 14)] == [GENERIC, GENERIC]
    assert [r['kernel'] for r in ops.roi_align_plan('forward', [(2796203, 3)], 2, 256, 512, 14)] == [GENERIC, GENERIC]
    with knobs(1):
        assert wsb(512, 14) == 0 and [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 256, 512, 14, workspace=512 * 32)] == [TILE]
    with knobs(2):
        assert wsb(1, 14) == 32 and [r['kernel'] for r in ops.roi_align_plan('forward', PYRAMID, 2, 256, 1, 14)] == [ORDER, TILE]
    assert wsb(1, 14) == 0


def test_band_and_generic_routes():
    # P = 56 on P2: the band kernel, one channel quad per workgroup: 256 / 4 = 64 chunks, launch order, the staging buffer +
    # the stencil table of 2 x 64 x 8 floats: (2048 + 256) float4
    one, = ops.roi_align_plan('forward', [(200, 336)], 2, 256, 128, 56)
    _is(one, kernel=BAND, P0=2048, P1=4, grid=128 * 64, threads=256, lds_bytes=(2048 + 256) * 16, CT=4, order=0, lds_floats=0, levels=1)
    for P, kernel in ((16, TILE), (17, BAND), (64, BAND), (65, GENERIC)):
        assert ops.roi_align_plan('forward', [(200, 336)], 2, 256, 128, P)[0]['kernel'] == kernel, P
    # a map column must fit 20 bits: W = 2^20 leaves the band kernel (and 2^23 pixels the tile kernel keeps)
    assert ops.roi_align_plan('forward', [(8, 1 << 20)], 2, 256, 128, 56)[0]['kernel'] == GENERIC
    assert ops.roi_align_plan('forward', [(8, 1 << 20)], 2, 256, 128, 14)[0]['kernel'] == TILE
    assert ops.roi_align_plan('forward', [(16, 1 << 19)], 2, 256, 128, 56)[0]['kernel'] == BAND
    # C % 4 != 0: the generic kernel, one launch per sampling-grid class, 16 channels per workgroup: 1 chunk of the 6
    # channels, 3 RoIs; 6 x 1024 LDS floats = 24576 bytes.  From 32 x 32 bins on (P x P >= 1024): 8 channels per workgroup
    a, b = ops.roi_align_plan('forward', PYRAMID, 2, 6, 3, 14)
    _is(a, kernel=GENERIC, P0=0, P1=1, grid=3, threads=256, lds_bytes=24576, CT=16, order=0, lds_floats=6144, levels=1)
    assert b == dict(a, P1=2)
    a, b = ops.roi_align_plan('forward', PYRAMID, 2, 256, 3, 112)
    _is(a, kernel=GENERIC, P0=0, P1=1, grid=3 * 32, CT=8, lds_floats=6144)
    assert ops.roi_align_plan('forward', PYRAMID, 2, 6, 3, 31)[0]['CT'] == 16 and ops.roi_align_plan('forward', PYRAMID, 2, 6, 3, 32)[0]['CT'] == 8


def test_backward_routes():
    # 16 < P <= 64 and channels in quads: the gather form, a quad per workgroup, LDS: P x P gradient quads + the tables of
    # 384 samples: 28 x 28 x 16 + 384 x 64 + 386 x 8 = 12544 + 24576 + 3088
    one, = ops.roi_align_plan('backward', [(200, 336)], 2, 256, 100, 28)
    _is(one, kernel=GATHER, P0=0, P1=0, grid=100 * 64, threads=256, lds_bytes=40208, CT=4, order=0, lds_floats=0, levels=0)
    # else the scatter form of the generic kernel: 16 channels per workgroup, 4 from 32 x 32 bins on; no dynamic LDS
    one, = ops.roi_align_plan('backward', PYRAMID, 2, 256, 100, 14)
    _is(one, kernel=GENERIC, P0=1, P1=0, grid=100 * 16, threads=256, lds_bytes=0, CT=16, order=0, lds_floats=0, levels=0)
    for P, C, kernel, ct in ((16, 256, GENERIC, 16), (17, 256, GATHER, 4), (64, 256, GATHER, 4), (65, 256, GENERIC, 4), (28, 6, GENERIC, 16),
                             (32, 6, GENERIC, 4)):
        _is(ops.roi_align_plan('backward', PYRAMID, 2, C, 100, P)[0], kernel=kernel, CT=ct)


def test_the_add_entry_takes_the_forward_plans_channels_per_workgroup(table):
    """The header's promise: dm_roi_align_add_fwd launches with the channels per workgroup -- and so the bits -- of the forward
    of the same RoIs with the workspace dm_roi_align_workspace_bytes asks for.  Over every add row of the table."""
    args, rcs, recs = table
    seen = set()
    for k in range(len(KNOBS)):
        with knobs(k):
            for i in np.nonzero((args[:, 20] == k) & (args[:, 0] == ADD))[0].tolist():
                a = args[i].tolist()
                pool, N, P = a[1], a[15], a[16]
                need = _lib.lib().dm_roi_align_workspace_bytes(N, P)
                frc, frec = _raw([FWD, 0] + a[2:18] + [need, 1 if need else 0])
                if rcs[i] == UNSUPPORTED:
                    # an odd P for the block means, a grid beyond 2^31 - 1, or a forward that does not take the tile kernel
                    assert (pool == 2 and P % 2) or frc == UNSUPPORTED or (frc >= 1 and frec[(frc - 1) * N_INTS] != TILE), a
                if rcs[i] < 1:
                    continue
                add, fwd = recs[i][:N_INTS].tolist(), frec[(frc - 1) * N_INTS:frc * N_INTS]
                assert rcs[i] == 1 and add[0] == fwd[0] == TILE and add[1] == a[1] and fwd[1] == 0, a
                assert add[3:9] == fwd[3:9], (a, add, fwd)                # grid, threads, LDS, CT, order, lds_floats
                assert add[9] == 0
                seen.add((a[1], add[6], frc))
    assert seen == {(1, 16, 1), (2, 16, 1), (1, 32, 2), (2, 32, 2)}
    # by hand: 200 RoIs order (CT 32, 64 / 32 = 2 chunks, launch order), 5 do not (CT 16, 4 chunks)
    _is(ops.roi_align_plan('add', [(50, 84)], 2, 64, 200, 14, pool=2)[0], kernel=TILE, P0=2, grid=400, CT=32, order=0, lds_bytes=TILE_LDS)
    _is(ops.roi_align_plan('add', [(50, 84)], 2, 64, 5, 14, pool=1)[0], kernel=TILE, P0=1, grid=20, CT=16, order=0)
    # N x chunks beyond 2^31 - 1: 2^27 RoIs x 16 chunks
    assert ops.roi_align_plan('add', [(50, 84)], 2, 256, (1 << 27) - 1, 14, pool=1)[0]['grid'] == ((1 << 27) - 1) * 16
    assert ops.roi_align_plan_raw('add', [(50, 84)], 2, 256, 1 << 27, 14, pool=1)[0] == UNSUPPORTED


ERRORS = [
    ('no level', dict(L=0), INVALID),
    ('five levels', dict(L=5), INVALID),
    ('B = 0', dict(B=0), INVALID),
    ('C = 0', dict(C=0), INVALID),
    ('N < 0', dict(N=-1), INVALID),
    ('P = 0', dict(P=0), INVALID),
    ('negative sampling ratio', dict(sr=-1), INVALID),
    ('an empty map', dict(H=(200, 0, 50, 25, 1)), INVALID),
    ('invalid before N = 0', dict(N=0, C=0), INVALID),
    ('bytes without a pointer', dict(wsb=64, ws=0), INVALID),
    ('negative bytes', dict(wsb=-1, ws=1), INVALID),
    ('workspace kind 3', dict(ws=3), INVALID),
    ('no such entry', dict(entry=3), INVALID),
    ('a workspace for the backward', dict(entry=BWD, wsb=64, ws=1), INVALID),
    ('a workspace for the add entry', dict(entry=ADD, pool=1, L=1, wsb=64, ws=1), INVALID),
    ('the add entry has one map', dict(entry=ADD, pool=1), INVALID),
    ('pool 3', dict(entry=ADD, pool=3, L=1), INVALID),
    ('pool 2 and odd P', dict(entry=ADD, pool=2, L=1, P=7), UNSUPPORTED),
    ('add: channels not in quads', dict(entry=ADD, pool=1, L=1, C=6), UNSUPPORTED),
    ('add: P = 28', dict(entry=ADD, pool=1, L=1, P=28), UNSUPPORTED),
    ('add: invalid before unsupported', dict(entry=ADD, pool=1, L=1, P=28, B=0), INVALID),
    ('one record of room', dict(cap=1), INVALID),
    ('null record array', dict(null=True), INVALID),
]


@pytest.mark.parametrize('name,change,code', ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_return_their_code_and_write_nothing(name, change, code):
    base = dict(entry=FWD, pool=0, L=4, H=(200, 100, 50, 25, 1), W=(336, 168, 84, 42, 1), B=2, C=256, N=512, P=14, sr=0, wsb=0, ws=0)
    row = lambda c: [c['entry'], c['pool'], c['L'], *c['H'], *c['W'], c['B'], c['C'], c['N'], c['P'], c['sr'], c['wsb'], c['ws']]   # noqa: E731
    ok, rec = _raw(row(base), fill=-77)
    assert ok == 1 and rec[N_INTS:] == [-77] * N_INTS and -77 not in rec[:N_INTS]
    call = dict(base, **change)
    rc, rec = _raw(row(call), cap=call.get('cap', N_REC), null=call.get('null', False), fill=-77)
    assert rc == code, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'
    if code == UNSUPPORTED:
        with pytest.raises(RuntimeError, match='dm_roi_align_plan'):
            ops.roi_align_plan('add', [(200, 336)], call['B'], call['C'], call['N'], call['P'], pool=call['pool'])
