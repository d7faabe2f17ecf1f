"""tests/support_cases.py against the library's own ``dm_*_supported`` predicates, on the host (the library loads without
a device): every row the sweep runs is accepted, every neighbour is refused, the finite sets are exactly what an
enumeration of the predicate over a box one step wider than its constants yields, the corners the tables promise are
present, and the tile constants the corners bracket are still the ones in the ``.hip`` sources."""
import ctypes
import itertools

import pytest

import support_cases as sc
from dynamask_amd import _lib


def _ask(name, row):
    fn = getattr(_lib.lib(), name)
    if name == 'dm_conv3x3_multidil_supported':
        dil = row[-1]
        return fn(*row[:-1], len(dil), (ctypes.c_int * len(dil))(*dil))
    return fn(*row)


@pytest.mark.parametrize('name', sorted(sc.TABLES))
def test_every_run_row_is_accepted_and_every_neighbour_refused(name):
    run, refused = sc.TABLES[name]
    assert run and refused, name
    assert len(set(run)) == len(run), f'{name}: a row is listed twice'
    for row in run:
        assert _ask(name, row) == 1, f'{name}{row}: listed to run, refused by the library'
    for row in refused:
        assert _ask(name, row) == 0, f'{name}{row}: listed as refused, accepted by the library'
    assert not set(run) & set(refused), name


@pytest.mark.parametrize('key', sorted(sc.TILE_CONSTANTS), ids=lambda k: f'{k[0]}:{k[1]}')
def test_tile_constants_are_the_sources(key):
    assert sc.hip_constant(*key) == sc.TILE_CONSTANTS[key], f'{key}: the kernel tiles differently now; revisit the tables'


def _wider(values):
    """Every integer from one below the smallest to one above the largest of ``values``."""
    return range(min(values) - 1, max(values) + 2)


def test_the_deconv_table_is_the_whole_accepted_set():
    L = _lib.lib()
    s = sc.DECONV_SETS
    box = itertools.product(_wider(s['G']), _wider(s['ci']), _wider(s['co']), _wider(s['S']))
    accepted = {r for r in box if L.dm_deconv4x4_s2_grouped_supported(2, *r) == 1}
    assert accepted == set(sc.DECONV_SHAPES) and len(sc.DECONV_SHAPES) == 48
    assert {r[1:] for r in sc.DECONV_RUN} == accepted and {r[0] for r in sc.DECONV_RUN} == {1, 2}
    assert len(sc.DECONV_RUN) == 96


def test_the_fusion_table_is_the_whole_accepted_set():
    L = _lib.lib()
    s = sc.FUSION_SETS
    box = itertools.product(_wider(s['P']), _wider(s['c']), _wider(s['S']))
    accepted = {r for r in box if L.dm_grid_fusion_supported(3, *r) == 1}
    assert accepted == set(sc.FUSION_SHAPES) and len(sc.FUSION_SHAPES) == 8
    assert {r[1:] for r in sc.FUSION_RUN} == accepted and {r[0] for r in sc.FUSION_RUN} == {1, 3}
    for P, c in itertools.product(_wider(s['P']), _wider(s['c'])):
        assert (L.dm_grid_fusion_table_floats(P, c) > 0) == (P in s['P'] and c in s['c'])


def _has(rows, **named):
    """Is there a row whose fields have the given values?  ``_3=8``: field 3 is 8."""
    at = {int(k[1:]): v for k, v in named.items()}
    return any(all(r[i] == v for i, v in at.items()) for r in rows)


def test_point_mlp_corners():
    TP = sc.TILE_CONSTANTS[('mfma_tile.h', 'DM_MLP_TP')]
    rows = sc.POINT_MLP_RUN
    for NC, nfc, P in itertools.product((8, 48, sc.TILE_CONSTANTS[('point_refine.hip', 'MLP_MAXNC')]),
                                        range(1, sc.TILE_CONSTANTS[('point_refine.hip', 'MLP_MAXFC')] + 1),
                                        (1, TP - 1, TP, TP + 1, 2 * TP + 1)):
        for HW in (P, P + 7):
            assert _has(rows, _1=P, _3=NC, _5=nfc, _7=HW), (NC, nfc, P, HW)
    assert {r[6] for r in rows} == {1, 2, 81} and all(r[0] >= 2 for r in rows)
    for nc in (0, 4, 104):
        assert _has(sc.POINT_MLP_REFUSED, _3=nc)
    for nfc in (0, 5):
        assert _has(sc.POINT_MLP_REFUSED, _5=nfc)
    assert any(r[1] == r[7] + 1 for r in sc.POINT_MLP_REFUSED)


def test_refine_mlp_corners():
    TP = sc.TILE_CONSTANTS[('mfma_tile.h', 'DM_MLP_TP')]
    rows = sc.REFINE_MLP_RUN
    maxnc = sc.TILE_CONSTANTS[('point_refine.hip', 'RMLP_MAXNC')]
    for C, NC, nfc in itertools.product((64, 128, 256), (8, 24, maxnc), (1, sc.TILE_CONSTANTS[('point_refine.hip', 'RMLP_MAXFC')])):
        for P in (1, TP - 1, TP, TP + 1):
            assert _has(rows, _1=P, _2=C, _3=NC, _4=nfc, _6=1), (C, NC, nfc, P)
        for HW in (1, 49, TP + 1):
            assert _has(rows, _1=HW, _2=C, _3=NC, _4=nfc, _5=HW, _6=0), (C, NC, nfc, HW)
    for nfc in (2, 3):
        assert _has(rows, _4=nfc)
    ref = sc.REFINE_MLP_REFUSED
    assert _has(ref, _2=96) and _has(ref, _3=maxnc + 8) and _has(ref, _2=64, _3=12)
    assert _has(ref, _4=5) and any(r[6] == 0 and r[1] != r[5] for r in ref)


def test_select_corners():
    NT = sc.TILE_CONSTANTS[('point_refine.hip', 'SEL_NT')]
    assert set(sc.SELECT_HW) >= {1, 2, 63, 64, 65, NT - 1, NT, NT + 1, 2 * NT + 1}
    for HW, n in itertools.product(sc.SELECT_HW, (1, 3)):
        for P in {1, (HW + 1) // 2, HW - 1, HW} - {0}:
            assert (n, HW, P) in sc.SELECT_RUN, (n, HW, P)
    top = sc.TILE_CONSTANTS[('point_refine.hip', 'SEL_MAX_HW')]
    assert sc.SELECT_BIG == (1, top, 1 << 12) and (1, top + 1, 1 << 12) in sc.SELECT_REFUSED


def test_gather_corners():
    CG, NT = sc.TILE_CONSTANTS[('point_refine.hip', 'GAT_CG')], sc.TILE_CONSTANTS[('point_refine.hip', 'GAT_NT')]
    g = sc.GATHER_RUN
    assert {r[1] for r in g} == {CG, 2 * CG, 256} and {r[5] for r in g} == {CG, 80}
    assert {(r[9], r[10]) for r in g} == {(1, 1), (3, 5), (28, 28)} and {(r[6], r[7]) for r in g} == {(1, 1), (7, 4)}
    assert all(r[0] == 2 and r[4] == sc.GATHER_N and r[2] != r[3] for r in g)
    assert any(NT < r[4] * r[8] < NT + 8 for r in g), 'no case one workgroup and a few points long'
    f = sc.FEAT_GATHER_RUN
    assert {r[1] for r in f} == {CG, 2 * CG, 256} and {r[5] for r in f} == {CG, 160}
    assert {(r[7], r[8]) for r in f} == {(S, h) for S in (1, 2, 7) for h in (0, 1)}
    assert all(r[6] == r[7] * r[7] for r in f if r[8] == 0)
    for rows, c, nc in ((sc.GATHER_REFUSED, 1, 5), (sc.FEAT_GATHER_REFUSED, 1, 5)):
        assert {r[c] for r in rows} >= {CG // 2, CG + CG // 2} and {r[nc] for r in rows} >= {CG // 2, CG + CG // 2}


def test_grid_and_conv_corners():
    assert set(sc.GET_BBOXES_RUN) == {(3, P, HS, D) for HS in (1, 2, 3, 56, 1024) for P in (4, 9) for D in (5, 6)}
    assert (3, 9, 1025, 5) in sc.GET_BBOXES_REFUSED and (3, 9, 56, 4) in sc.GET_BBOXES_REFUSED
    TN, MAXS = sc.TILE_CONSTANTS[('conv_strided.hip', 'S2_TN')], sc.TILE_CONSTANTS[('conv_strided.hip', 'S2_MAXSPLIT')]
    s2 = sc.CONV_S2_RUN
    assert all(r[5] != 0 for r in s2 + sc.CONV_S2_REFUSED), 'splits = 0 depends on the CU count'
    for C in (8, 16, 64):
        admitted = [s for s in (1, 2, 4, 8) if s <= C // 8 and s <= MAXS]
        for (H, W), cout, s in itertools.product(sc.S2_MAPS, sc.COUT_EDGES, admitted):
            assert (2, C, H, W, cout, s) in s2
        first_refused = 2 * admitted[-1]
        assert _has(sc.CONV_S2_REFUSED, _1=C, _5=first_refused), (C, first_refused)
    pixels = {r[0] * ((r[2] + 1) // 2) * ((r[3] + 1) // 2) for r in s2}
    assert pixels >= {2, TN - 1, TN, TN + 1, 2 * TN}          # (2: one output pixel per image)
    TH, TW = sc.TILE_CONSTANTS[('conv_dilated.hip', 'DIL_TH')], sc.TILE_CONSTANTS[('conv_dilated.hip', 'DIL_TW')]
    for d in range(1, sc.TILE_CONSTANTS[('conv_dilated.hip', 'DIL_MAXD')] + 1):
        for H, W in ((1, 1), (d, d), (d + 1, 2 * d + 1), (TH + 1, TW + 1)):
            assert _has(sc.DIL_RUN, _2=H, _3=W, _5=d), (d, H, W)
    assert {r[4] for r in sc.DIL_RUN} >= set(sc.COUT_EDGES) and {r[4] for r in s2} >= set(sc.COUT_EDGES)
    assert any(r[5] == (1, 8, 3) for r in sc.MULTIDIL_RUN)
    assert {(r[2], r[3]) for r in sc.MASK_IOU_RUN} == {(2, 2), (2, 5), (13, 28)}
    assert {r[2] for r in sc.GAP_RUN} == {1, 255, 256, 257, 4099} and {r[0] * r[1] for r in sc.GAP_RUN} == {1, 3, 4, 5, 1027}


def test_the_capped_launchers_still_cap():
    """Every launcher of the table still holds its cap, wherever the line has moved to."""
    for name, (fname, _, _, cap) in sc.CAPPED.items():
        line, text = sc.capped_line(name)
        print(f'{name}: {fname}:{line} caps at {cap}')
        assert str(cap) in text, (name, text)


def test_select_cut_tie_inputs_tie_at_the_cut():
    """The planted group really holds the cut: fewer better keys than P, and more keys up to the group than P."""
    import torch
    for mode in sc.SELECT_MODES:
        for _, HW, P in sc.SELECT_RUN:
            m = sc.cut_tie_map(mode, HW, P, torch.Generator().manual_seed(HW + P))
            key = m.abs() if mode == 'mag' else -m
            cut = torch.sort(key).values[P - 1]
            n_eq, n_lt = int((key == cut).sum()), int((key < cut).sum())
            assert 2 <= n_eq <= 8 or HW == 1          # (eight cells; fewer where the map ends inside the group)
            assert n_lt < P <= n_lt + n_eq
            if HW > 1024:
                eq = torch.nonzero(key == cut).view(-1)
                assert int(eq.min()) < 1024 <= int(eq.max())


def test_the_split_k_finish_case_splits_and_passes_the_cap():
    """The shape the sweep runs for the split-K finishes: both launchers split it (asked at 256 compute units, the count
    the library assumes without a device and the MI355X's), and its outputs are more than 4096 x 256 float4."""
    from dynamask_amd import ops
    L = _lib.lib()
    NB, C, H, W, cout = sc.SPLITK_FINISH_CASE
    per = NB * cout * H * W
    assert per % 4 == 0 and per // 4 > sc.CAPPED['dm_conv2d_fwd_ws/reduce'][3] * 256
    nws = L.dm_conv2d_splitk_floats(NB, H, W, cout, 3)
    rec, = ops.conv2d_plan([C], NB, H, W, cout, 3, workspace_floats=nws)
    assert rec['ksplit'] >= 2 and rec['grid_y'] == rec['ksplit']
    dws = L.dm_deform_conv_splitk_floats(NB, C, H, W, cout)
    drec = ops.deform_conv_plan(NB, C, H, W, cout, 2, workspace_floats=dws)
    assert drec[0]['reduce'] == 1 and drec[0]['ksplit'] >= 2
