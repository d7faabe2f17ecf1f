"""The shapes the point, grid and head kernels are run at by tests/test_support_sweep_gpu.py, and the neighbours just past
each boundary that their ``dm_*_supported`` predicates must refuse.  Host only: no device (``cut_tie_map`` builds a CPU tensor).

A row is the argument tuple of the entry point's predicate, in the predicate's own order, so test_support_cases_cpu.py
can ask the library about every row on a machine without a GPU and the sweep can unpack the same row on the device.
Where the accepted set is finite (the grouped deconvolution, the neighbour fusion) the table is the whole set, enumerated;
where it is open the table holds the corners: every parameter at its smallest and largest accepted value and at both
sides of each constant the kernel tiles by.  Those constants are read from the ``.hip`` sources by ``hip_constant`` and
pinned in ``TILE_CONSTANTS`` with the line they stand on, so a kernel whose tile changes fails the CPU test until the
table has been looked at again."""
import itertools
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dynamask_amd', 'csrc')


def hip_constant(filename, name):
    """The value of ``constexpr <type> ... NAME = <integer expression>`` in csrc/<filename> (digits, shifts, products)."""
    with open(os.path.join(CSRC, filename)) as f:
        for no, line in enumerate(f, 1):
            m = re.search(r'\b%s\s*=\s*([^,;]+)[,;]' % re.escape(name), line) if 'constexpr' in line else None
            if m:
                expr = re.sub(r'(\d+)(?:LL|ll|u|U)\b', r'\1', m.group(1).strip())
                if not re.fullmatch(r'[\d\s<>()*+/-]+', expr):
                    raise ValueError(f'{filename}:{no}: {name} = {expr!r} is not a plain integer expression')
                return int(eval(expr, {'__builtins__': {}}))      # noqa: S307 (digits and operators only)
    raise KeyError(f'{name} not found in {filename}')


# (file, name): value -- the constants the tables below bracket, with the line each was read from.
TILE_CONSTANTS = {
    ('mfma_tile.h', 'DM_MLP_TP'): 64,                 # :116  points per workgroup of both point MLPs
    ('point_refine.hip', 'SEL_NT'): 1024,             # :28   keys per tile of the select's compaction loop
    ('point_refine.hip', 'SEL_MAX_HW'): 1 << 24,      # :31
    ('point_refine.hip', 'GAT_NT'): 256,              # :147  points per workgroup of both gathers
    ('point_refine.hip', 'GAT_CG'): 8,                # :148  channels per gather thread
    ('point_refine.hip', 'MLP_MAXFC'): 4,             # :229
    ('point_refine.hip', 'MLP_MAXNC'): 96,            # :230
    ('point_refine.hip', 'RMLP_MAXNC'): 160,          # :452
    ('point_refine.hip', 'RMLP_MAXFC'): 4,            # :453
    ('grid_head.hip', 'DECONV_MAX_CI'): 64,           # :419
    ('grid_head.hip', 'DECONV_MAX_S'): 14,            # :419
    ('conv_strided.hip', 'S2_TN'): 64,                # :28   output pixels per workgroup of the stride-2 conv
    ('conv_strided.hip', 'S2_MAXSPLIT'): 8,           # :31
    ('conv_dilated.hip', 'DIL_TH'): 8,                # :29   the 8 x 16 = 128-pixel block of the dilated conv
    ('conv_dilated.hip', 'DIL_TW'): 16,               # :29
    ('conv_dilated.hip', 'DIL_MAXD'): 8,              # :31
}
# Cout tiles of the 3x3 launches (mfma_tile.h:180 dm_cout_tiles): the packed cout count is a multiple of 32, a workgroup
# takes 64 couts of a map of <= 64 and 128 otherwise -- hence Cout 1 / 33 / 64 / 65 below.
COUT_EDGES = (1, 33, 64, 65)


def _uniq(rows):
    out = []
    for r in rows:
        if r not in out:
            out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ dm_point_mlp_fwd
# predicate (n, P, C, NC, F, num_fcs, NCL, HW).  P 1 / 63 / 64 / 65 / 129: one point, one short of, exactly, one past a
# DM_MLP_TP = 64 tile, and three tiles with a one-point tail.  HW = P (every cell is a point) and P + 7.  Two RoIs, so the
# labels 0 and NCL - 1 are both present; NCL 1 (class-agnostic), 2, 81 go round with P.
MLP_NCL_OF_P = {1: 81, 63: 1, 64: 2, 65: 81, 129: 2}
POINT_MLP_RUN = [(2, P, 256, NC, 256, nfc, MLP_NCL_OF_P[P], HW)
                 for NC in (8, 48, 96) for nfc in (1, 2, 3, 4) for P in (1, 63, 64, 65, 129) for HW in (P, P + 7)]
POINT_MLP_RUN += [(2, 65, 256, 48, 256, 3, ncl, 72) for ncl in (1, 2)]       # every NCL at the tile-and-one-point shape too
POINT_MLP_REFUSED = [(2, 64, 256, nc, 256, 3, 81, 71) for nc in (0, 4, 104)]
POINT_MLP_REFUSED += [(2, 64, 256, 48, 256, nfc, 81, 71) for nfc in (0, 5)]
POINT_MLP_REFUSED += [(2, 72, 256, 48, 256, 3, 81, 71),                       # P = HW + 1
                      (2, 0, 256, 48, 256, 3, 81, 71), (2, 64, 256, 48, 256, 3, 0, 71),
                      (2, 64, 128, 48, 256, 3, 81, 71), (2, 64, 256, 48, 128, 3, 81, 71), (-1, 64, 256, 48, 256, 3, 81, 71)]

# ------------------------------------------------------------------------------------------------ dm_point_refine_mlp
# predicate (n, P, C, NC, num_fcs, HW, has_idx).  C picks the wave layout (point_refine.hip:467-470), NC 8 / 24 / 160
# the smallest, an odd multiple of 8 and RMLP_MAXNC; with an index array P brackets the 64-point tile in a 72-cell map,
# without one P = HW.
REFINE_CNF = [(C, NC, nfc) for C in (64, 128, 256) for NC in (8, 24, 160) for nfc in (1, 4)] + [(128, 24, 2), (128, 24, 3)]
REFINE_HW_IDX = 72
REFINE_MLP_RUN = [(2, P, C, NC, nfc, REFINE_HW_IDX, 1) for C, NC, nfc in REFINE_CNF for P in (1, 63, 64, 65)]
REFINE_MLP_RUN += [(2, HW, C, NC, nfc, HW, 0) for C, NC, nfc in REFINE_CNF for HW in (1, 49, 65)]
REFINE_MLP_REFUSED = [(2, 64, 96, 24, 2, 72, 1), (2, 64, 64, 168, 2, 72, 1), (2, 64, 64, 12, 2, 72, 1), (2, 64, 64, 24, 5, 72, 1),
                      (2, 64, 64, 24, 2, 72, 0),                               # P != HW without an index array
                      (2, 64, 64, 0, 2, 72, 1), (2, 64, 64, 24, 0, 72, 1), (2, 73, 64, 24, 2, 72, 1), (2, 0, 64, 24, 2, 72, 1),
                      (2, 64, 512, 24, 2, 72, 1)]

# ------------------------------------------------------------------------------------------------ the selects
# predicate (n, HW, P) -- dm_point_topk_select_supported appends the mode.  HW brackets one wave (64), the SEL_NT = 1024
# tile of the compaction loop and its third trip (2049); P is 1, half, all but one and all of the cells.
SELECT_HW = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049)
SELECT_RUN = _uniq([(n, HW, P) for HW in SELECT_HW for n in (1, 3) for P in sorted({1, (HW + 1) // 2, HW - 1, HW}) if P >= 1])
SELECT_BIG = (1, 1 << 24, 1 << 12)                    # the largest map the predicate takes, one row
SELECT_REFUSED = [(1, (1 << 24) + 1, 1 << 12), (1, 64, 65), (1, 64, 0), (1, 0, 1), (-1, 64, 8)]
SELECT_MODES = ('mag', 'raw', 'sigmoid')              # dm_point_select; dm_point_topk_select mode 0; mode 1
TOPK_MODE_REFUSED = [(1, 64, 8, 2), (1, 64, 8, -1)]


def cut_tie_map(mode, HW, P, g):
    """Distinct keys except one group of equal ones that the cut at P falls into; the group lies across index 1024 (the
    edge of the first SEL_NT tile) where the map has one, else across the middle."""
    import torch
    c = 1024 if HW > 1024 else HW // 2
    tied = torch.arange(max(c - 4, 0), min(c + 4, HW))
    nt = len(tied)
    better = min(max(P - max(nt // 2, 1), 0), HW - nt)
    rest = torch.tensor(sorted(set(range(HW)) - set(tied.tolist())), dtype=torch.long)
    rest = rest[torch.randperm(len(rest), generator=g)]
    rank = torch.empty(HW)
    rank[rest[:better]] = torch.arange(better, dtype=torch.float32)
    rank[tied] = float(better)
    rank[rest[better:]] = torch.arange(better + 1, HW - nt + 1, dtype=torch.float32)
    if mode == 'mag':                       # smallest |v| first; the signs are mixed
        sign = torch.where(torch.rand(HW, generator=g) < 0.5, -1.0, 1.0)
        return (rank + 1) * 2.0 ** -10 * sign
    if mode == 'raw':                       # largest v first
        return (HW / 2 - rank) * 2.0 ** -10
    return 4.0 - rank * (8.0 / HW)          # sigmoid: a step of 8 / 2049 moves the logistic by >= 7e-5, hundreds of ulps


# ------------------------------------------------------------------------------------------------ dm_point_gather_fwd
# predicate (B, C, H, W, n, NC, CH, CW, P, MH, MW).  C / NC: one GAT_CG = 8 group, two, and the heads' counts; the feature
# map 6 x 9, the coarse map 1 x 1 and 7 x 4, the point grid 1 x 1, 3 x 5 and 28 x 28, all independent and non-square.
# Five RoIs (images 0, 1, one outside the batch, partly and wholly outside the map); P = 1, every cell, and at 28 x 28 also
# 52: 5 x 52 = 260 points, one GAT_NT = 256 workgroup and four points.
GATHER_N = 5
GATHER_RUN = []
for _C, _NC in ((8, 8), (16, 80), (256, 8), (256, 80)):
    for (_CH, _CW), (_MH, _MW) in itertools.product(((1, 1), (7, 4)), ((1, 1), (3, 5), (28, 28))):
        for _P in sorted({1, _MH * _MW} | ({52} if _MH == 28 else set())):
            GATHER_RUN.append((2, _C, 6, 9, GATHER_N, _NC, _CH, _CW, _P, _MH, _MW))
GATHER_REFUSED = [(2, 4, 6, 9, 5, 8, 7, 4, 15, 3, 5), (2, 12, 6, 9, 5, 8, 7, 4, 15, 3, 5), (2, 8, 6, 9, 5, 4, 7, 4, 15, 3, 5),
                  (2, 8, 6, 9, 5, 12, 7, 4, 15, 3, 5), (2, 8, 6, 9, 5, 8, 7, 4, 16, 3, 5), (2, 8, 6, 9, 5, 8, 7, 4, 0, 3, 5),
                  (0, 8, 6, 9, 5, 8, 7, 4, 15, 3, 5), (2, 8, 0, 9, 5, 8, 7, 4, 15, 3, 5), (2, 8, 6, 9, 5, 8, 0, 4, 15, 3, 5),
                  (2, 8, 6, 9, 5, 8, 7, 4, 1, 0, 5), (2, 8, 6, 9, -1, 8, 7, 4, 15, 3, 5)]

# ------------------------------------------------------------------------------------------------ dm_point_feat_gather
# predicate (B, C, H, W, n, NC, P, S, has_idx).  S 1 / 2 / 7; without an index array P = S * S, with one P = 1 and
# S * S - 1 (S * S at S = 1).
FEAT_GATHER_RUN = []
for _C, _NC in ((8, 8), (16, 160), (256, 8), (256, 160)):
    for _S in (1, 2, 7):
        FEAT_GATHER_RUN.append((2, _C, 6, 9, GATHER_N, _NC, _S * _S, _S, 0))
        for _P in sorted({1, max(_S * _S - 1, 1)}):
            FEAT_GATHER_RUN.append((2, _C, 6, 9, GATHER_N, _NC, _P, _S, 1))
FEAT_GATHER_REFUSED = [(2, 4, 6, 9, 5, 8, 4, 2, 1), (2, 12, 6, 9, 5, 8, 4, 2, 1), (2, 8, 6, 9, 5, 4, 4, 2, 1),
                       (2, 8, 6, 9, 5, 12, 4, 2, 1), (2, 8, 6, 9, 5, 8, 5, 2, 1), (2, 8, 6, 9, 5, 8, 3, 2, 0),
                       (2, 8, 6, 9, 5, 8, 0, 2, 1), (2, 8, 6, 9, 5, 8, 1, 0, 1), (0, 8, 6, 9, 5, 8, 4, 2, 1),
                       (2, 8 * 65535, 6, 9, 5, 8, 4, 2, 1)]           # (C + NC) / 8 channel groups past the grid's y limit

# ------------------------------------------------------------------------------------------------ the Grid head
# dm_deconv4x4_s2_grouped_supported (N, G, ci, co, S): G {4, 9} x ci {8, 64} x co {1, 8, 64} x S {1, 3, 7, 14}
# (grid_head.hip:424-427), every one of the 48 for N 1 and 2.
DECONV_SETS = dict(G=(4, 9), ci=(8, 64), co=(1, 8, 64), S=(1, 3, 7, 14))
DECONV_SHAPES = list(itertools.product(DECONV_SETS['G'], DECONV_SETS['ci'], DECONV_SETS['co'], DECONV_SETS['S']))
DECONV_RUN = [(N,) + s for s in DECONV_SHAPES for N in (1, 2)]
DECONV_REFUSED = [(2, 3, 8, 8, 7), (2, 5, 8, 8, 7), (2, 8, 8, 8, 7), (2, 10, 8, 8, 7), (2, 9, 7, 8, 7), (2, 9, 9, 8, 7), (2, 9, 63, 8, 7),
                  (2, 9, 65, 8, 7), (2, 9, 8, 0, 7), (2, 9, 8, 2, 7), (2, 9, 8, 7, 7), (2, 9, 8, 9, 7), (2, 9, 8, 63, 7), (2, 9, 8, 65, 7),
                  (2, 9, 8, 8, 0), (2, 9, 8, 8, 2), (2, 9, 8, 8, 4), (2, 9, 8, 8, 6), (2, 9, 8, 8, 8), (2, 9, 8, 8, 13),
                  (2, 9, 8, 8, 15), (-1, 9, 8, 8, 7)]
# dm_grid_fusion_supported (N, P, c, S): P {4, 9} x c {8, 64} x S {3, 7} (grid_head.hip:414), all 8 for N 1 and 3.
FUSION_SETS = dict(P=(4, 9), c=(8, 64), S=(3, 7))
FUSION_SHAPES = list(itertools.product(FUSION_SETS['P'], FUSION_SETS['c'], FUSION_SETS['S']))
FUSION_RUN = [(N,) + s for s in FUSION_SHAPES for N in (1, 3)]
FUSION_REFUSED = [(3, 3, 8, 7), (3, 5, 8, 7), (3, 8, 8, 7), (3, 10, 8, 7), (3, 16, 8, 7), (3, 9, 7, 7), (3, 9, 9, 7), (3, 9, 63, 7),
                  (3, 9, 65, 7), (3, 9, 8, 2), (3, 9, 8, 4), (3, 9, 8, 6), (3, 9, 8, 8), (-1, 9, 8, 7)]
# dm_grid_get_bboxes_supported (n, P, HS, D): a one-cell map, maps below the 256-thread workgroup (grid_head.hip GH_NT),
# the config's 56 and the largest accepted; three samples (maximum in the first cell, in the last, tied).
GET_BBOXES_RUN = [(3, P, HS, D) for HS in (1, 2, 3, 56, 1024) for P in (4, 9) for D in (5, 6)]
GET_BBOXES_REFUSED = [(3, 9, 0, 5), (3, 9, 1025, 5), (3, 9, 56, 4), (3, 3, 56, 5), (3, 5, 56, 5), (3, 8, 56, 5), (3, 10, 56, 5),
                      (3, 16, 56, 5), (-1, 9, 56, 5)]

# ------------------------------------------------------------------------------------------------ dm_conv3x3_s2_fwd
# predicate (NB, C, H, W, Cout, splits).  Explicit splits only (0 resolves by the device's CU count): every one of 1, 2, 4,
# 8 that C / 8 chunks admit, and the first one past them.  Maps 1 x 1, 2 x 3, 13 x 14 (2 x 49 = 98 output pixels: a ragged
# second S2_TN = 64 tile) and 15 x 15 (2 x 64: two exact tiles); one image of 13 x 17 / 15 x 15 / 9 x 25 gives 63 / 64 / 65.
S2_MAPS = ((1, 1), (2, 3), (13, 14), (15, 15))
S2_SPLITS = {8: (1,), 16: (1, 2), 64: (1, 2, 4, 8)}
CONV_S2_RUN = [(2, C, H, W, cout, s) for C in (8, 16, 64) for (H, W) in S2_MAPS for cout in COUT_EDGES for s in S2_SPLITS[C]]
CONV_S2_RUN += [(1, 16, H, W, 33, 2) for (H, W) in ((13, 17), (15, 15), (9, 25))]
CONV_S2_REFUSED = [(2, 8, 13, 14, 33, 2), (2, 16, 13, 14, 33, 4), (2, 64, 13, 14, 33, 16), (2, 64, 13, 14, 33, 3),
                   (2, 32, 13, 14, 33, 8), (2, 64, 13, 14, 33, -1), (0, 64, 13, 14, 33, 1), (2, 4, 13, 14, 33, 1),
                   (2, 12, 13, 14, 33, 1), (2, 64, 0, 14, 33, 1), (2, 64, 13, 0, 33, 1), (2, 64, 13, 14, 0, 1)]

# ------------------------------------------------------------------------------------------------ dm_conv3x3_dil_fwd
# predicate (NB, C, H, W, Cout, dilation).  Every dilation 1 .. DIL_MAXD on a 1 x 1 map (all eight off-centre taps are
# padding), d x d (the off-centre taps just miss the map), (d + 1) x (2 d + 1) (they just reach it) and 9 x 17 (one pixel
# past the 8 x 16 block in both directions: four workgroups per image); the cout tile edges at one dilation.
DIL_RUN = _uniq([(2, 16, H, W, 40, d) for d in range(1, 9) for (H, W) in ((1, 1), (d, d), (d + 1, 2 * d + 1), (9, 17))])
DIL_RUN += [(2, 8, 9, 17, cout, 2) for cout in COUT_EDGES]
DIL_REFUSED = [(2, 16, 9, 17, 40, 0), (2, 16, 9, 17, 40, 9), (2, 4, 9, 17, 40, 1), (2, 12, 9, 17, 40, 1), (0, 16, 9, 17, 40, 1),
               (2, 16, 0, 17, 40, 1), (2, 16, 9, 0, 40, 1), (2, 16, 9, 17, 0, 1)]
# dm_conv3x3_multidil_supported (NB, C, H, W, Cout, (dilations)): three branches of mixed dilations.
MULTIDIL_RUN = [(2, 16, H, W, 40, (1, 8, 3)) for (H, W) in ((1, 1), (5, 7), (9, 17))] + [(1, 8, 9, 17, 65, (8, 1, 8))]
MULTIDIL_REFUSED = [(2, 16, 9, 17, 40, (1, 8)), (2, 16, 9, 17, 40, (1, 8, 3, 1)), (2, 16, 9, 17, 40, (1, 9, 3)),
                    (2, 16, 9, 17, 40, (0, 8, 3)), (2, 12, 9, 17, 40, (1, 8, 3))]

# ------------------------------------------------------------------------------------------------ pooled
# dm_mask_iou_input_supported (n, C, H, W): the smallest map, an odd width (the last column is dropped), 13 x 28.
MASK_IOU_RUN = [(3, C, H, W) for C in (1, 80) for (H, W) in ((2, 2), (2, 5), (13, 28))]
MASK_IOU_REFUSED = [(3, 80, 1, 28), (3, 80, 28, 1), (3, 0, 28, 28), (-1, 80, 28, 28)]
# dm_global_avg_pool_supported (N, C, HW): HW brackets 256 = four trips of the 64 lanes (pointwise.hip:1289) and 4099;
# N * C brackets the four planes of a workgroup (pointwise.hip:1284) and 1027 = 13 x 79.
GAP_RUN = [(N, C, HW) for HW in (1, 255, 256, 257, 4099) for (N, C) in ((1, 1), (3, 1), (1, 4), (5, 1), (13, 79))]
GAP_REFUSED = [(2, 4, 0), (2, 4, (1 << 24) + 1), (2, 0, 49), (-1, 4, 49), (1 << 20, 1 << 12, 49)]

# ------------------------------------------------------------------------------------------------ the capped grids
# Launchers that cap their grid and walk the rest in a loop: name -> (file, the text that opens the launcher, the cap as
# the source writes it, the cap's value).  ``capped_line`` finds the cap's line (the first line after the opening text
# that holds the cap inside a min(...) or a conditional); the lines below are where that was on the day of writing.
# The sweep runs each at the smallest tensor whose item count passes cap * 256.  An item is what one thread makes per
# trip: four outputs of a row for the max-pool (stem.hip:308 WoG) and the generic x2 upsample (pointwise.hip:340 OWq), two
# input pixels (eight outputs) for the half-pixel build, a float4 for dm_relu_bwd's aligned build and the split-K finishes,
# a whole plane for the LDS builds of the x2 upsample's adjoint (cap: 8 workgroups per compute unit), one output elsewhere.
CAPPED = {
    'dm_maxpool3x3_s2_fwd': ('stem.hip', 'int dm_maxpool3x3_s2_fwd(', '65536', 65536),                          # :310
    'dm_resize_bilinear_fwd': ('pointwise.hip', 'int dm_resize_bilinear_fwd(', '65536', 65536),                 # :999
    'dm_upsample2x_bilinear_fwd/half': ('pointwise.hip', 'int dm_upsample2x_bilinear_fwd(', '65536', 65536),    # :983
    'dm_upsample2x_bilinear_fwd/generic': ('pointwise.hip', 'int dm_upsample2x_bilinear_fwd(', '32768', 32768),  # :988
    'dm_subsample2_fwd': ('pointwise.hip', 'int dm_subsample2_fwd(', '16384', 16384),                           # :1332
    'dm_avgpool2x2_ceil_fwd': ('pointwise.hip', 'int dm_avgpool2x2_ceil_fwd(', '16384', 16384),                 # :1372
    'dm_threshold_ge': ('pointwise.hip', 'int dm_threshold_ge(', '16384', 16384),                               # :1236
    'dm_sgd_momentum_step': ('api_misc.hip', 'int dm_sgd_momentum_step(', '4096', 4096),                        # :53
    'dm_sumsq': ('bbox_train.hip', 'int dm_sumsq(', '1024', 1024),             # :496  workgroups of 16384 elements, not 256
    'dm_merge_aug_masks': ('rle.hip', 'int dm_merge_aug_masks(', '8192', 8192),                                 # :409
    'grid_for': ('backward.hip', 'int grid_for(', '16384', 16384),             # :1866  dm_relu_bwd (:1874, :1878),
    #                                  dm_sigmoid_bwd (:1886), the gather and scatter routes of the x2 upsample's adjoint (:2209, :2217)
    'dm_upsample2x_bilinear_bwd/lds': ('backward.hip', 'BwdRoute upsample_bwd_route(', '8 * c.cus', 8),        # :2203  per CU
    'dm_conv2d_fwd_ws/reduce': ('conv_igemm.hip', 'int launch_splitk_reduce(', '4096', 4096),                   # :1274
    'dm_deform_conv_fwd_ws/reduce': ('deform_conv.hip', 'int dcn_emit(', '4096', 4096),                         # :1428
}
# dm_scale (bbox_train.hip:513) launches ceil(count / 256) workgroups, one element per thread: there is no cap to pass.
# The split-K finishes pass their cap from 4 Mi outputs on, and a launch splits only while its workgroups fill less than a
# round of the chip: 100 RoIs of 14 x 14 at 256 -> 256 channels (5 017 600 outputs, 4900 workgroups' worth) do both, for
# the 3x3 convolution (two splits, conv_igemm.hip:1589-1594) and for the DCN (three, deform_conv.hip:1262-1267).
SPLITK_FINISH_CASE = (100, 256, 14, 14, 256)          # NB, C, H, W, Cout


def capped_line(name):
    """(line number, text) of the cap of launcher ``name`` in today's source."""
    fname, opening, cap_text, _ = CAPPED[name]
    with open(os.path.join(CSRC, fname)) as f:
        lines = f.read().splitlines()
    start = next(i for i, ln in enumerate(lines) if opening in ln)
    for i in range(start, min(start + 40, len(lines))):
        if cap_text in lines[i] and ('min(' in lines[i] or '?' in lines[i]):
            return i + 1, lines[i]
    raise LookupError(f'{name}: no cap {cap_text!r} within 40 lines of {opening!r} in {fname}')


TABLES = {
    'dm_point_mlp_supported': (POINT_MLP_RUN, POINT_MLP_REFUSED),
    'dm_point_refine_mlp_supported': (REFINE_MLP_RUN, REFINE_MLP_REFUSED),
    'dm_point_select_supported': (SELECT_RUN + [SELECT_BIG], SELECT_REFUSED),
    'dm_point_topk_select_supported': ([r + (m,) for r in SELECT_RUN + [SELECT_BIG] for m in (0, 1)],
                                       [r + (m,) for r in SELECT_REFUSED for m in (0, 1)] + TOPK_MODE_REFUSED),
    'dm_point_gather_supported': (GATHER_RUN, GATHER_REFUSED),
    'dm_point_feat_gather_supported': (FEAT_GATHER_RUN, FEAT_GATHER_REFUSED),
    'dm_deconv4x4_s2_grouped_supported': (DECONV_RUN, DECONV_REFUSED),
    'dm_grid_fusion_supported': (FUSION_RUN, FUSION_REFUSED),
    'dm_grid_get_bboxes_supported': (GET_BBOXES_RUN, GET_BBOXES_REFUSED),
    'dm_conv3x3_s2_supported': (CONV_S2_RUN, CONV_S2_REFUSED),
    'dm_conv3x3_dil_supported': (DIL_RUN, DIL_REFUSED),
    'dm_conv3x3_multidil_supported': (MULTIDIL_RUN, MULTIDIL_REFUSED),
    'dm_mask_iou_input_supported': (MASK_IOU_RUN, MASK_IOU_REFUSED),
    'dm_global_avg_pool_supported': (GAP_RUN, GAP_REFUSED),
}
