"""dm_conv2d_plan: the convolution launcher's own report of what it would launch (csrc/conv_igemm.hip: conv2d_launch runs
with a recorder and launches nothing), pinned at the 256-CU fallback of a machine without a device for the shapes the
project's numbers rest on.  Every expected value below is worked out from conv2d_launch by hand, in the comment next to
it.  No GPU needed; on a machine WITH a device the compute-unit count is the device's and the CU-dependent pins are
skipped (tests/test_conv_builds_gpu.py holds them against the device's count there)."""
import ctypes

import pytest

from dynamask_amd import _abi, _lib, ops

CONSTS = _abi.load()[1]
N_INTS, N_REC = CONSTS['DM_CONV_PLAN_INTS'], CONSTS['DM_CONV_PLAN_MAX_LAUNCHES']
INVALID, UNSUPPORTED = CONSTS['DM_ERR_INVALID_ARG'], CONSTS['DM_ERR_UNSUPPORTED']

B128 = dict(KS=3, WGM=2, WGN=2, WM=2, WN=2, CK=8, TAIL=0, PREC=0, POST=0)       # 128 couts x 128 pixels
B32 = dict(KS=3, WGM=4, WGN=1, WM=1, WN=1, CK=8, TAIL=0, PREC=0, POST=0)        # 128 couts x 32 pixels
B64 = dict(KS=3, WGM=1, WGN=4, WM=2, WN=1, CK=8, TAIL=0, PREC=0, POST=0)        # 64 couts x 128 pixels
B32C = dict(KS=3, WGM=1, WGN=4, WM=1, WN=1, CK=8, TAIL=0, PREC=0, POST=0)       # 32 couts x 128 pixels
BTAIL = dict(B32C, TAIL=4)                                                      # 32 + 4 couts x 128 pixels
P1_SMALL = dict(KS=1, WGM=4, WGN=1, WM=1, WN=1, CK=32, TAIL=0, PREC=0, POST=0)
P1_128 = dict(KS=1, WGM=2, WGN=2, WM=2, WN=2, CK=16, TAIL=0, PREC=0, POST=0)
P1_64 = dict(KS=1, WGM=2, WGN=2, WM=1, WN=2, CK=16, TAIL=0, PREC=0, POST=0)
P1_32 = dict(KS=1, WGM=1, WGN=4, WM=1, WN=1, CK=32, TAIL=0, PREC=0, POST=0)


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


needs_256 = pytest.mark.skipif(_cus() != 256, reason='pins worked out for the 256-CU count the library assumes without a device')


def _is(rec, build, **more):
    want = dict(build, **more)
    got = {k: rec[k] for k in want}
    assert got == want, (got, want)


def test_record_layout_and_field_names():
    assert N_INTS == len(ops.CONV_PLAN_FIELDS) == 17 and N_REC == 2
    assert ops.conv2d_plan([256], 0, 14, 14, 256, 3) == []            # NB = 0: DM_OK, nothing launched


@needs_256
def test_headline_3x3_main_and_tail_launch():
    # 512 x 256 x 14 x 14 -> 256: Q = 100352 = 784 tiles of 128 px, CoutP = 256 -> MT = 2, 1568 workgroups.  The plane of a
    # 128-px tile: rmax = ceil(127/14) + 1 + 2 (ceil(127/196) + 1) = 15 rows of 16 -> 240 <= 256: MAXPOS 1, three workgroups
    # per CU, 768 slots.  1568 = 2 x 768 + 32: two full rounds, rem = 32, 32 x 5 <= 3 x 768 -> the seam.  n_main = 2 x 768 / 2
    # = 768 pixel tiles = 98304 px; the last 2048 px go to 64 tiles of 32 px x MT 2 = 128 workgroups of the 128 x 32 build,
    # whose plane is (ceil(31/14) + 1 + 4) x 16 = 128 <= 256: MAXPOS 1.
    main, tail = ops.conv2d_plan([256], 512, 14, 14, 256, 3)
    _is(main, B128, MAXPOS=1, ksplit=1, kchunks=0, q_begin=0, Q=98304, grid_x=1536, grid_y=1, nontemporal=0)
    _is(tail, B32, MAXPOS=1, ksplit=1, kchunks=0, q_begin=98304, Q=100352, grid_x=128, grid_y=1, nontemporal=0)
    # flag bit 3 (the caller overlaps another stream): one launch
    one, = ops.conv2d_plan([256], 512, 14, 14, 256, 3, overlapped=True)
    _is(one, B128, MAXPOS=1, q_begin=0, Q=100352, grid_x=1568, grid_y=1)
    # ReLU does not enter the decision; accumulate neither (3x3)
    assert ops.conv2d_plan([256], 512, 14, 14, 256, 3, relu=True) == [main, tail]
    assert ops.conv2d_plan([256], 512, 14, 14, 256, 3, accumulate=True) == [main, tail]
    assert ops.conv2d_plan([256], 512, 14, 14, 256, 3, has_mask=True) == [main, tail]


@needs_256
def test_small_3x3_launches_take_the_128x32_build():
    # 7 RoIs: 1372 px = 11 tiles x MT 2 = 22 workgroups, 22 x 10 <= 256 x 7 -> 128 x 32 tiles: 43 x 2 = 86
    one, = ops.conv2d_plan([256], 7, 14, 14, 256, 3)
    _is(one, B32, MAXPOS=1, q_begin=0, Q=1372, grid_x=86, grid_y=1)
    # first clause's edge: wgs x 10 <= 1792 <=> wgs <= 179; MT 2 -> 89 tiles (NB 58: 11368 px = 89 tiles), 90 tiles (NB 59:
    # 11564 px = 91 tiles -> 182 workgroups <= 256 CUs: neither clause) -> 128 x 128
    _is(ops.conv2d_plan([256], 58, 14, 14, 256, 3)[0], B32, grid_x=2 * 356)
    r = ops.conv2d_plan([256], 59, 14, 14, 256, 3)
    assert len(r) == 1
    _is(r[0], B128, grid_x=182)
    # second clause: 256 < wgs, wgs x 20 <= 7424 <=> wgs <= 371.  NB 100: 19600 px = 154 tiles, 308 workgroups -> 128 x 32;
    # NB 122: 23912 px = 187 tiles, 374 workgroups -> 128 x 128
    _is(ops.conv2d_plan([256], 100, 14, 14, 256, 3)[0], B32, grid_x=2 * 613)
    r = ops.conv2d_plan([256], 122, 14, 14, 256, 3)
    assert len(r) == 1
    _is(r[0], B128, grid_x=374)


@needs_256
def test_seam_threshold_and_two_per_cu_maps():
    # 28 x 28 maps: rmax = ceil(127/28) + 1 + 4 = 10 rows of 30 = 300 > 256 -> MAXPOS 2, two per CU, 512 slots.  Cout 130 ->
    # CoutP 160 -> MT 2.  rem x 5 <= 1536 <=> rem <= 307.  NB 52: 40768 px = 319 tiles (318.5), 638 = 512 + 126 -> seam at
    # n_main = 256 tiles = 32768 px (41.8 images: inside an image).  NB 67: 52528 px = 411 tiles (410.4), 822 = 512 + 310 -> none.
    main, tail = ops.conv2d_plan([8, 3, 1], 52, 28, 28, 130, 3)
    _is(main, B128, MAXPOS=2, Q=32768, grid_x=512)
    _is(tail, B32, MAXPOS=1, q_begin=32768, Q=40768, grid_x=2 * 250)
    assert 32768 % (28 * 28) != 0
    one, = ops.conv2d_plan([8, 3, 1], 67, 28, 28, 130, 3)
    _is(one, B128, MAXPOS=2, Q=52528, grid_x=822)
    # (rem 306 / 308 would need 409 / 410 tiles, and no multiple of 784 px ends in either: NB 66 and 67 are the rule's
    # two sides on this map)
    main, tail = ops.conv2d_plan([8, 3, 1], 66, 28, 28, 130, 3)          # 51744 px = 405 tiles (404.25), 810 = 512 + 298
    _is(main, B128, Q=32768)
    _is(tail, B32, q_begin=32768, Q=51744)


@needs_256
def test_3x3_builds_by_cout_and_staged_depth():
    for cout, build in ((33, BTAIL), (36, BTAIL), (37, B64), (64, B64), (1, B32C), (32, B32C)):
        one, = ops.conv2d_plan([20], 3, 14, 14, cout, 3)
        _is(one, build, MAXPOS=1, grid_x=5, Q=588)
    # accumulating launches of 33 .. 36 couts go to the 64-cout build; masked ones keep the tail rows' build
    for cout in (33, 36):
        _is(ops.conv2d_plan([20], 3, 14, 14, cout, 3, accumulate=True)[0], B64)
        _is(ops.conv2d_plan([20], 3, 14, 14, cout, 3, has_mask=True)[0], BTAIL)
    # staged depth, 128-px tiles of 256 threads: plane = (ceil(127/W) + 1 + 2 (ceil(127/HW) + 1)) (W + 2)
    #   14 x 14: 240 -> 1;  56 x 56: (3 + 1 + 4) x 58 = 464 -> 2;  5 x 120: (2 + 1 + 4) x 122 = 854 -> 4;
    #   1 x 14: (10 + 1 + 2 x 11) x 16 = 528 -> 4;  3 x 1: (127 + 1 + 2 x 44) x 3 = 648 -> 4
    for (H, W), mp in (((14, 14), 1), ((56, 56), 2), ((5, 120), 4), ((1, 14), 4), ((3, 1), 4)):
        for cout, build in ((36, BTAIL), (64, B64), (32, B32C)):
            _is(ops.conv2d_plan([20], 2, H, W, cout, 3)[0], build, MAXPOS=mp)
    # 128 x 32 tiles (NT 256 too): 9 x 112: (1 + 1 + 4) x 114 = 684 -> 4; 2 x 2: (16 + 1 + 2 x 9) x 4 = 140 -> 1 while the
    # 128-px tile of the same map stages (64 + 1 + 2 x 33) x 4 = 524 -> 4
    _is(ops.conv2d_plan([12], 2, 9, 112, 65, 3)[0], B32, MAXPOS=4)
    _is(ops.conv2d_plan([16], 8, 2, 2, 96, 3)[0], B32, MAXPOS=1)
    _is(ops.conv2d_plan([16], 8, 2, 2, 96, 3, overlapped=True)[0], B32, MAXPOS=1)
    # 2 x 2, Cout 96 (MT 1): 128 x 128 from 372 tiles on -> NB 32 x 372 = 11904 images
    _is(ops.conv2d_plan([16], 11904, 2, 2, 96, 3)[0], B128, MAXPOS=4, grid_x=372)


@needs_256
def test_1x1_builds_and_the_tile_threshold():
    # (5 x 256) / 4 = 320 tiles of 128 x 128.  Cout 256: MT 2 -> 160 pixel tiles = 20480 px: NB 104 (20384 px, 160 tiles) is
    # the last small launch, NB 105 (20580 px, 161 tiles) the first 128 x 128 one
    _is(ops.conv2d_plan([256], 104, 14, 14, 256, 1)[0], P1_SMALL, MAXPOS=1, grid_x=2 * 637, Q=20384)
    _is(ops.conv2d_plan([256], 105, 14, 14, 256, 1)[0], P1_128, MAXPOS=1, grid_x=2 * 161, Q=20580)
    # Cout 65 .. 128: MT 1 -> 320 pixel tiles = 40960 px: NB 208 (40768 px, 319 tiles), 209 (40964 px: 321 tiles)
    for cout in (65, 126, 128):
        _is(ops.conv2d_plan([72], 208, 14, 14, cout, 1)[0], P1_SMALL, grid_x=1274)
        _is(ops.conv2d_plan([72], 209, 14, 14, cout, 1)[0], P1_128, grid_x=321)
    # Cout 130: CoutP 160 -> MT 2 again
    _is(ops.conv2d_plan([72], 104, 14, 14, 130, 1)[0], P1_SMALL)
    _is(ops.conv2d_plan([72], 105, 14, 14, 130, 1)[0], P1_128)
    # accumulating and masked launches never take the small build; the post-add launch takes its own twin of each
    _is(ops.conv2d_plan([72], 3, 14, 14, 130, 1, accumulate=True)[0], P1_128)
    _is(ops.conv2d_plan([72], 3, 14, 14, 130, 1, has_mask=True)[0], P1_128)
    _is(ops.conv2d_plan([72], 3, 14, 14, 130, 1, has_addend=True)[0], dict(P1_SMALL, POST=1))
    _is(ops.conv2d_plan([72], 105, 14, 14, 130, 1, has_addend=True)[0], dict(P1_128, POST=1))
    for cout, build in ((33, P1_64), (64, P1_64), (1, P1_32), (32, P1_32)):
        _is(ops.conv2d_plan([24, 8, 1, 1], 5, 33, 33, cout, 1)[0], build, MAXPOS=1, grid_x=43, Q=5445)
        _is(ops.conv2d_plan([24, 8, 1, 1], 5, 33, 33, cout, 1, has_addend=True)[0], dict(build, POST=1))


@needs_256
def test_workspace_path_splits_where_splitk_floats_says():
    L = _lib.lib()
    per = lambda nb, cout, hw: nb * cout * hw
    # 100 RoIs, 3x3 256 -> 256 @14: 308 tiles of 128 x 128, 2 x 308 <= 768 -> room for min(8, 768 / 308) = 2 splits; the cost
    # model: 32 chunks x 2.1 us x (1 - 1/2) = 33.6 us saved, 5 + 3 x 20.07 MB x 0.25 = 20.05 us paid: 13.5 > 8 -> 2 splits of 16
    assert L.dm_conv2d_splitk_floats(100, 14, 14, 256, 3) == 2 * per(100, 256, 196)
    one, = ops.conv2d_plan([256], 100, 14, 14, 256, 3, workspace_floats=2 * per(100, 256, 196))
    _is(one, B128, MAXPOS=1, ksplit=2, kchunks=16, grid_x=308, grid_y=2, Q=19600)
    # a workspace with room for one copy only: no split, and then the 128 x 32 tiles of the launch without a workspace
    one, = ops.conv2d_plan([256], 100, 14, 14, 256, 3, workspace_floats=2 * per(100, 256, 196) - 1)
    _is(one, B32, ksplit=1, kchunks=0, grid_y=1)
    # 16 RoIs: 50 tiles, min(8, 768 / 50) = 8 splits allowed, 32 / 4 = 8 by the chunk count; the model's gain grows up to 8
    # (58.8 - 12.2 = 46.6 us): 8 splits of 4 chunks
    assert L.dm_conv2d_splitk_floats(16, 14, 14, 256, 3) == 8 * per(16, 256, 196)
    one, = ops.conv2d_plan([256], 16, 14, 14, 256, 3, workspace_floats=8 * per(16, 256, 196))
    _is(one, B128, ksplit=8, kchunks=4, grid_x=50, grid_y=8)
    # the split never needs more than the workspace it was given, and never happens where splitk_floats says 0
    for nb in (1, 3, 16, 50, 100, 150, 196, 197, 250, 512):
        for cins, cout, ks, hw in (([256], 256, 3, 14), ([256], 36, 3, 14), ([128], 128, 3, 28), ([256, 256, 2], 256, 1, 14),
                                   ([64], 64, 3, 56)):
            want = L.dm_conv2d_splitk_floats(nb, hw, hw, cout, ks)
            recs = ops.conv2d_plan(cins, nb, hw, hw, cout, ks, workspace_floats=1 << 40)
            if want == 0:
                assert all(r['ksplit'] == 1 for r in recs), (nb, cins, cout, ks, hw)
            else:
                assert len(recs) == 1
                got = ops.conv2d_plan(cins, nb, hw, hw, cout, ks, workspace_floats=want)
                assert got == recs, 'more workspace than dm_conv2d_splitk_floats changes the plan'
                assert got[0]['ksplit'] * per(nb, cout, hw * hw) <= want
                assert got[0]['grid_y'] == got[0]['ksplit'] and (got[0]['kchunks'] > 0) == (got[0]['ksplit'] > 1)
    # a split launch has no seam
    assert ops.conv2d_plan([256], 196, 14, 14, 256, 3, workspace_floats=1 << 40)[0]['q_begin'] == 0


@needs_256
def test_nontemporal_bit_above_192_mb_of_output():
    # 192 MB = 50331648 floats; 64 couts x 56 x 56 = 200704 per image: NB 250 -> 50176000 (below), NB 251 -> 50376704 (above)
    assert ops.conv2d_plan([8], 250, 56, 56, 64, 1)[0]['nontemporal'] == 0
    assert ops.conv2d_plan([8], 251, 56, 56, 64, 1)[0]['nontemporal'] == 1
    assert ops.conv2d_plan([8], 251, 56, 56, 64, 3)[0]['nontemporal'] == 1
    assert ops.conv2d_plan([8], 251, 56, 56, 64, 1, accumulate=True)[0]['nontemporal'] == 0      # reads the destination
    assert all(r['nontemporal'] == 1 for r in ops.conv2d_plan([8], 251, 56, 56, 65, 3))


# (W = 168: the 128-px and the 32-px tile both stage (1 + 1 + 2 x 2) x 170 = 1020 <= 4 x 256 positions; W = 169: 6 x 171 = 1026)
WIDE = [(256, 2, B32), (256, 150, B128), (36, 2, BTAIL), (64, 2, B64), (32, 2, B32C)]


@needs_256
@pytest.mark.parametrize('cout,nb,build', WIDE)
def test_maps_168_wide_are_accepted_and_169_refused(cout, nb, build):
    # (Cout 256, NB 150, H 1: 25200 px = 197 tiles x MT 2 = 394 workgroups > 1.45 x 256 -> the 128 x 128 build)
    for H in (1, 3):
        if build is B128 and H != 1:
            continue
        rc, recs = ops.conv2d_plan_raw([8], nb, H, 168, cout, 3)
        assert rc == 1
        _is(recs[0], build, MAXPOS=4)
        assert ops.conv2d_plan_raw([8], nb, H, 169, cout, 3) == (UNSUPPORTED, [])
        assert ops.conv2d_plan_raw([8], nb, H, 169, cout, 1)[0] == 1              # 1x1 has no plane


def test_3x3_on_1x1_maps_does_not_depend_on_nb():
    # the 128-px tile would stage (127 + 1 + 2 x 128) x 3 = 1152 > 1024 positions, the 32-px tile (31 + 1 + 2 x 32) x 3 = 288:
    # Cout > 64 takes the 128 x 32 build for every NB, Cout <= 64 (128-px tiles only) is refused
    for nb in (1, 3, 300, 3000, 40000, 200000):
        for flags in (0, 8):
            rc, recs = ops.conv2d_plan_raw([8], nb, 1, 1, 96, 3, flags)
            assert rc == 1, (nb, flags)
            _is(recs[0], B32, MAXPOS=2, q_begin=0, Q=nb)
        assert ops.conv2d_plan_raw([8], nb, 1, 1, 96, 3, workspace_floats=1 << 40)[0] == 1
        for cout in (64, 36, 32):
            assert ops.conv2d_plan_raw([8], nb, 1, 1, cout, 3) == (UNSUPPORTED, [])


def _raw(src_channels, strides, num_srcs, NB, H, W, cout, ksize, flags, oct_, oco, ws=0, mask=0, addend=0, cap=N_REC, null=False):
    """dm_conv2d_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_REC))(*([-77] * (N_INTS * N_REC)))
    sc = None if src_channels is None else (ctypes.c_int * len(src_channels))(*src_channels)
    sb = None if strides is None else (ctypes.c_longlong * len(strides))(*strides)
    rc = _lib.lib().dm_conv2d_plan(sc, sb, num_srcs, NB, H, W, cout, ksize, flags, oct_, oco, ws, mask, addend, None if null else rec, cap)
    return rc, list(rec)


ERRORS = [
    ('null src_channels', dict(src_channels=None), INVALID),
    ('no source', dict(num_srcs=0), INVALID),
    ('five sources', dict(src_channels=[8] * 5, num_srcs=5), INVALID),
    ('NB < 0', dict(NB=-1), INVALID),
    ('H = 0', dict(H=0), INVALID),
    ('W = 0', dict(W=0), INVALID),
    ('Cout = 0', dict(cout=0), INVALID),
    ('ksize 2', dict(ksize=2), INVALID),
    ('ksize 5', dict(ksize=5), INVALID),
    ('channel offset < 0', dict(oco=-1), INVALID),
    ('slice past the tensor', dict(oct_=256, oco=1), INVALID),
    ('2^31 pixels', dict(NB=1 << 20, H=64, W=32), INVALID),
    ('empty source', dict(src_channels=[8, 0], num_srcs=2), INVALID),
    ('batch stride shorter than the source', dict(strides=[256 * 196 - 1]), INVALID),
    ('flag bit 2', dict(flags=4), INVALID),
    ('flag bit 2 with others', dict(flags=1 | 4 | 8), INVALID),
    ('flag bit 5', dict(flags=32), INVALID),
    ('flag bit 6', dict(flags=64), INVALID),
    ('bf16x3 with a mask', dict(flags=16, mask=1), UNSUPPORTED),
    ('addend on 3x3', dict(addend=1), UNSUPPORTED),
    ('addend with bf16x3', dict(ksize=1, flags=16, addend=1), UNSUPPORTED),
    ('addend with accumulate', dict(ksize=1, flags=2, addend=1), INVALID),
    ('addend with the stream hint', dict(ksize=1, flags=8, addend=1), INVALID),
    ('addend and mask', dict(ksize=1, mask=1, addend=1), INVALID),
    ('mask with a workspace', dict(mask=1, ws=1 << 30), INVALID),
    ('negative workspace', dict(ws=-1), INVALID),
    ('bf16x3 3x3 on 28 x 28', dict(flags=16, H=28, W=28), UNSUPPORTED),
    ('map 169 wide', dict(W=169), UNSUPPORTED),
    ('map 169 wide behind a full-size main launch', dict(NB=2000, H=2, W=169), UNSUPPORTED),
    ('3x3, 64 couts on 1x1 maps', dict(H=1, W=1, cout=64, oct_=64), UNSUPPORTED),
    ('one record of room', dict(cap=1), INVALID),
    ('null record array', dict(null=True), INVALID),
]


@pytest.mark.parametrize('name,change,code', ERRORS, ids=[e[0] for e in ERRORS])
def test_error_paths_return_their_code_and_write_nothing(name, change, code):
    base = dict(src_channels=[256], strides=None, num_srcs=1, NB=512, H=14, W=14, cout=256, ksize=3, flags=0, oct_=256, oco=0)
    ok, rec = _raw(**base)
    assert ok >= 1 and rec[0] == 3 and rec[ok * N_INTS:] == [-77] * ((N_REC - ok) * N_INTS)       # the base call is a valid one
    rc, rec = _raw(**dict(base, **change))
    assert rc == code, name
    assert rec == [-77] * (N_INTS * N_REC), 'a partial record was left behind'


def test_accepted_flag_bits_are_0_1_3_4():
    for flags in (0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 24, 25):
        rc, _ = ops.conv2d_plan_raw([256], 7, 14, 14, 256, 3, flags)
        assert rc == 1, flags
    for flags in (4, 5, 6, 7, 12, 20, 32, 33, 64, 128, 1 << 30, -1):
        assert ops.conv2d_plan_raw([256], 7, 14, 14, 256, 3, flags)[0] == INVALID, flags
    one, = ops.conv2d_plan([256], 7, 14, 14, 256, 3, bf16x3=True)
    _is(one, dict(KS=3, WGM=2, WGN=2, WM=1, WN=2, CK=16, TAIL=0, PREC=1, POST=0), MAXPOS=1)


# ---------------------------------------------------------------------------------------------------------------------
# dm_conv2d_group_plan: the grouped launcher (dm_conv2d_group_fwd) under the same recorder -- one record per problem of the
# ONE launch: grid_x the problem's share of the grid, the split shared.  Worked out from dm_conv2d_group_fwd by hand.
N_GREC = CONSTS['DM_CONV_GROUP_PLAN_MAX']


def _gplan(count, NB, H, W, cin, cout, ksize, ws=0, **kw):
    """The records of a grouped call, after the properties every grouped plan has: `count` equal records, no seam, the
    split dm_conv2d_group_splits reports for the same arguments."""
    recs = ops.conv2d_group_plan(count, NB, H, W, cin, cout, ksize, workspace_floats=ws, **kw)
    assert len(recs) == count and all(r == recs[0] for r in recs)
    S = _lib.lib().dm_conv2d_group_splits(count, NB, H, W, cin, cout, ksize, ws)
    r = recs[0]
    assert r['ksplit'] == r['grid_y'] == S and r['q_begin'] == 0 and r['Q'] == NB * H * W
    assert (r['kchunks'] > 0) == (S > 1)
    return r


def test_group_record_room():
    assert N_GREC == 3 and N_GREC >= N_REC
    assert ops.conv2d_group_plan(3, 0, 14, 14, 256, 256, 3) == []          # NB = 0: DM_OK, nothing launched


@needs_256
def test_group_3x3_splits_on_the_grouped_workgroup_count():
    L = _lib.lib()
    per = 16 * 256 * 196              # 802816 floats = 3.21 MB per problem
    # 16 RoIs, 256 -> 256 @14: Q = 3136 = 25 tiles of 128 px (24.5) x MT 2 = 50 workgroups per problem; plane 15 x 16 = 240:
    # MAXPOS 1.  The grouped 128 x 128 build runs two per CU: 512 slots.  32 chunks of 8 channels, 32 / 4 = 8 splits at most.
    # count 3: 150 workgroups, 512 / 150 = 3 splits; the model: 67.2 us x 2/3 = 44.8 saved, 5 + 4 x 3.21 MB x 0.25 = 8.2 paid:
    # 36.6 us, above two splits' 33.6 - 7.4 = 26.2 -> 3 splits of ceil(32 / 3) = 11 chunks
    assert L.dm_conv2d_group_splitk_floats(3, 16, 14, 14, 256, 256, 3) == 3 * 3 * per
    _is(_gplan(3, 16, 14, 14, 256, 256, 3, ws=9 * per), B128, MAXPOS=1, ksplit=3, kchunks=11, grid_x=50, grid_y=3, nontemporal=0)
    assert _gplan(3, 16, 14, 14, 256, 256, 3, ws=1 << 40) == _gplan(3, 16, 14, 14, 256, 256, 3, ws=9 * per)
    # one float less: room for two splits per problem -> 2 splits of 16
    _is(_gplan(3, 16, 14, 14, 256, 256, 3, ws=9 * per - 1), B128, ksplit=2, kchunks=16, grid_x=50, grid_y=2)
    # count 1: 50 workgroups, min(8, 512 / 50) = 8; the gain grows up to 8 (58.8 - 12.2 = 46.6 us): 8 splits of 4
    assert L.dm_conv2d_group_splitk_floats(1, 16, 14, 14, 256, 256, 3) == 8 * per
    _is(_gplan(1, 16, 14, 14, 256, 256, 3, ws=8 * per), B128, MAXPOS=1, ksplit=8, kchunks=4, grid_x=50, grid_y=8)
    # no workspace, or one too small for two splits: no split, and 150 (50) x 10 <= 1792 -> the 128 x 32 build, 98 tiles of
    # 32 px x MT 2 = 196 workgroups per problem, plane (3 + 1 + 4) x 16 = 128: MAXPOS 1
    for count, ws in ((3, 0), (1, 0), (3, 6 * per - 1), (1, 2 * per - 1)):
        _is(_gplan(count, 16, 14, 14, 256, 256, 3, ws=ws), B32, MAXPOS=1, ksplit=1, kchunks=0, grid_x=196, grid_y=1)
    # a grid that fills the slots does not split: NB 100, count 3: 3 x 308 = 924 >= 512
    assert L.dm_conv2d_group_splitk_floats(3, 100, 14, 14, 256, 256, 3) == 0
    _is(_gplan(3, 100, 14, 14, 256, 256, 3, ws=1 << 40), B128, ksplit=1, grid_x=308)


@needs_256
def test_group_small_launch_rule_both_clauses():
    # count x MT x tiles workgroups against 256 CUs.  First clause: wgs x 10 <= 1792 <=> wgs <= 179.
    # count 1 (the lone launch's numbers): NB 58: 89 tiles, 178 -> 128 x 32 (356 tiles of 32 px x 2); NB 59: 91 tiles, 182 -> 128 x 128
    _is(_gplan(1, 58, 14, 14, 256, 256, 3), B32, grid_x=712)
    _is(_gplan(1, 59, 14, 14, 256, 256, 3), B128, grid_x=182)
    # count 3: NB 18: 3528 px = 28 tiles (27.6), 3 x 56 = 168 -> 128 x 32 (111 tiles x 2); NB 19: 3724 px = 30 tiles, 180 -> 128 x 128
    _is(_gplan(3, 18, 14, 14, 256, 256, 3), B32, grid_x=222)
    _is(_gplan(3, 19, 14, 14, 256, 256, 3), B128, grid_x=60)
    # second clause: 256 < wgs and wgs x 20 <= 7424 <=> wgs <= 371.  count 1: NB 100: 308 -> 128 x 32 (613 x 2); NB 122: 374 -> 128 x 128
    _is(_gplan(1, 100, 14, 14, 256, 256, 3), B32, grid_x=1226)
    _is(_gplan(1, 122, 14, 14, 256, 256, 3), B128, grid_x=374)
    # count 3: NB 39: 7644 px = 60 tiles (59.7), 360 -> 128 x 32 (239 tiles x 2); NB 40: 7840 px = 62 tiles (61.25), 372 -> 128 x 128
    _is(_gplan(3, 39, 14, 14, 256, 256, 3), B32, grid_x=478)
    _is(_gplan(3, 40, 14, 14, 256, 256, 3), B128, grid_x=124)
    # between the clauses (179 < wgs <= 256): 128 x 128.  count 2, NB 25: 4900 px = 39 tiles (38.3), 156 -> 128 x 32;
    # NB 32: 6272 px = 49 tiles, 196 -> 128 x 128
    _is(_gplan(2, 25, 14, 14, 256, 256, 3), B32, grid_x=2 * 154)
    _is(_gplan(2, 32, 14, 14, 256, 256, 3), B128, grid_x=98)


@needs_256
def test_group_3x3_builds_by_cout_and_staged_depth():
    for cout, build in ((37, B64), (64, B64), (1, B32C), (32, B32C)):
        _is(_gplan(2, 3, 14, 14, 20, cout, 3), build, MAXPOS=1, grid_x=5, Q=588)
        _is(_gplan(2, 3, 14, 14, 20, cout, 3, ws=1 << 40), build, ksplit=1)         # 3 chunks: 3 / 4 = 0 splits
    # the 32 + 4 tail build has no grouped form
    for cout in (33, 34, 35, 36):
        assert ops.conv2d_group_plan_raw(2, 3, 14, 14, 20, cout, 3) == (UNSUPPORTED, [])
        _is(_gplan(2, 3, 14, 14, 20, cout, 1), P1_64)
    # staged depth (the planes of test_3x3_builds_by_cout_and_staged_depth): 14 x 14: 240 -> 1; 56 x 56: 464 -> 2; 5 x 120: 854 -> 4
    for (H, W), mp, tiles in (((14, 14), 1, 4), ((56, 56), 2, 49), ((5, 120), 4, 10)):
        for cout, build in ((64, B64), (32, B32C)):
            _is(_gplan(3, 2, H, W, 20, cout, 3), build, MAXPOS=mp, grid_x=tiles)
    # the 128 x 128 build on 28 x 28 maps: 10 rows of 30 = 300 -> MAXPOS 2; 16 x 784 px = 98 tiles x MT 2, 3 x 196 = 588 workgroups
    _is(_gplan(3, 16, 28, 28, 256, 256, 3), B128, MAXPOS=2, grid_x=196)
    # the 128 x 32 build (few workgroups): 9 x 112: (1 + 1 + 4) x 114 = 684 -> 4; 2016 px = 63 tiles x MT 1
    _is(_gplan(1, 2, 9, 112, 12, 65, 3), B32, MAXPOS=4, grid_x=63)
    # 64-cout launches split on three slots per CU (768): 256 -> 64 @14 x 16 RoIs, count 3: 3 x 25 = 75 workgroups, min(8, 10, 32 / 4)
    # = 8 splits; per = 16 x 64 x 196 = 200704 floats = 0.80 MB: the gain grows up to 8 (58.8 - 5 - 9 x 0.2 = 52.0 us)
    _is(_gplan(3, 16, 14, 14, 256, 64, 3, ws=1 << 40), B64, ksplit=8, kchunks=4, grid_x=25, grid_y=8)
    assert _lib.lib().dm_conv2d_group_splitk_floats(3, 16, 14, 14, 256, 64, 3) == 8 * 3 * 200704


@needs_256
def test_group_128x32_plane_is_held_to_64_kb():
    # The 128 x 32 build keeps an A image of 9 x 2 x 128 words (36 KB) beside the plane's 32 bytes per position: more than 896
    # positions need more than 64 KB.  The lone launcher raises that build's limit to 80 KB (test_maps_168_wide_...); the
    # grouped launcher refuses.  1 x 147: (1 + 1 + 2 x 2) x 149 = 894 positions; 1 x 148: 6 x 150 = 900; 1 x 168: 1020.
    _is(_gplan(2, 2, 1, 147, 8, 256, 3), B32, MAXPOS=4, grid_x=2 * 10)           # 294 px = 10 tiles of 32 (9.2)
    for W in (148, 168):
        assert ops.conv2d_group_plan_raw(2, 2, 1, W, 8, 256, 3) == (UNSUPPORTED, [])
        assert ops.conv2d_plan_raw([8], 2, 1, W, 256, 3)[0] == 1
    # the 128 x 128 build of the same maps has no A image: 2 x 16 x 1020 bytes
    _is(_gplan(3, 150, 1, 168, 8, 256, 3), B128, MAXPOS=4, grid_x=394)
    assert ops.conv2d_group_plan_raw(3, 150, 1, 169, 8, 256, 3) == (UNSUPPORTED, [])


@needs_256
def test_group_1x1_builds_never_split():
    # 3 x 196 = 588 px = 5 tiles of 128; Cout 130 -> CoutP 160 -> MT 2 of the 128-cout build; no small build in a grouped launch
    for ws in (0, 1 << 40):
        _is(_gplan(2, 3, 14, 14, 72, 130, 1, ws=ws), P1_128, MAXPOS=1, ksplit=1, kchunks=0, grid_x=10, grid_y=1)
        _is(_gplan(3, 3, 14, 14, 72, 65, 1, ws=ws), P1_128, grid_x=5)
        for cout, build in ((33, P1_64), (64, P1_64), (1, P1_32), (32, P1_32)):
            _is(_gplan(3, 3, 14, 14, 72, cout, 1, ws=ws), build, MAXPOS=1, ksplit=1, kchunks=0, grid_x=5, grid_y=1)
        _is(_gplan(1, 16, 14, 14, 256, 256, 1, ws=ws), P1_128, ksplit=1, grid_x=50)
    assert _lib.lib().dm_conv2d_group_splitk_floats(1, 16, 14, 14, 256, 256, 1) == 0


@needs_256
def test_group_nontemporal_bit_above_192_mb_of_output():
    # per problem, as test_nontemporal_bit_above_192_mb_of_output: 64 x 56 x 56 x NB 250 below, NB 251 above
    assert _gplan(2, 250, 56, 56, 8, 64, 1)['nontemporal'] == 0
    assert _gplan(2, 251, 56, 56, 8, 64, 1)['nontemporal'] == 1
    assert _gplan(2, 251, 56, 56, 8, 64, 3)['nontemporal'] == 1


def _graw(count=3, NB=16, H=14, W=14, cin=256, cout=256, ksize=3, flags=0, ws=0, cap=N_GREC, null=False):
    """dm_conv2d_group_plan straight through ctypes, the record array filled with a canary."""
    rec = (ctypes.c_int * (N_INTS * N_GREC))(*([-77] * (N_INTS * N_GREC)))
    rc = _lib.lib().dm_conv2d_group_plan(count, NB, H, W, cin, cout, ksize, flags, ws, None if null else rec, cap)
    return rc, list(rec)


GROUP_ERRORS = [
    ('no problem', dict(count=0), INVALID),
    ('four problems', dict(count=4), INVALID),
    ('NB < 0', dict(NB=-1), INVALID),
    ('H = 0', dict(H=0), INVALID),
    ('W = 0', dict(W=0), INVALID),
    ('Cin = 0', dict(cin=0), INVALID),
    ('Cout = 0', dict(cout=0), INVALID),
    ('ksize 2', dict(ksize=2), INVALID),
    ('ksize 5', dict(ksize=5), INVALID),
    ('2^31 pixels', dict(NB=1 << 20, H=64, W=32), INVALID),
    ('accumulate', dict(flags=2), INVALID),
    ('flag bit 2', dict(flags=4), INVALID),
    ('flag bit 5', dict(flags=32), INVALID),
    ('bf16x3', dict(flags=16), UNSUPPORTED),
    ('bf16x3 on 1x1', dict(flags=17, ksize=1), UNSUPPORTED),
    ('the tail build', dict(cout=34), UNSUPPORTED),
    ('negative workspace', dict(ws=-1), INVALID),
    ('map 169 wide', dict(W=169), UNSUPPORTED),
    ('128 x 32 plane above 64 KB', dict(NB=2, H=1, W=168), UNSUPPORTED),
    ('64 couts on 1x1 maps', dict(H=1, W=1, cout=64), UNSUPPORTED),
    ('two records of room', dict(cap=2), INVALID),
    ('null record array', dict(null=True), INVALID),
]


@pytest.mark.parametrize('name,change,code', GROUP_ERRORS, ids=[e[0] for e in GROUP_ERRORS])
def test_group_error_paths_return_their_code_and_write_nothing(name, change, code):
    ok, rec = _graw()
    assert ok == 3 and rec[0] == 3 and -77 not in rec                       # the base call is a valid one
    ok, rec = _graw(count=1, flags=1 | 8)                                    # (ReLU, and the ignored stream hint)
    assert ok == 1 and rec[N_INTS:] == [-77] * (2 * N_INTS)
    rc, rec = _graw(**change)
    assert rc == code, name
    assert rec == [-77] * (N_INTS * N_GREC), 'a partial record was left behind'
