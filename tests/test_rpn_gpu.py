"""RPN inference on the MI355X: the three post-processing kernels bit for bit against compositions of launches that existed
before them (``ops.sigmoid`` + a stable ``torch.sort``; ``AnchorGenerator.grid_anchors`` + gathers + ``ops.bbox_decode``; a
concatenation + a stable sort), ``RPNHead.forward`` / ``get_bboxes`` against the reference's own float32 and float64 runs
(tests/golden/g26_rpn.npz), the fused path against the composed one, and the chain into StandardRoIHead."""
import json
import os

import numpy as np
import pytest
import torch

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _hw(n):
    """H x W = n with H the largest divisor up to sqrt(n)."""
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def _map(A, hw, seed, kind='normal'):
    H, W = _hw(hw)
    x = torch.randn(A, H, W, generator=_g(seed)) * 3
    if kind == 'coarse':            # a grid of 13 values: many exact ties
        x = torch.round(x.clamp(-3, 3) * 2) / 2
    return x.cuda()


def _select_ref(ops, maps, nms_pre):
    """Per map: (indices, scores) of the stable descending sort of the library's own sigmoid, cut at K."""
    out = []
    for m in maps:
        s = ops.sigmoid(m.permute(1, 2, 0).reshape(-1).contiguous())
        ranked, order = torch.sort(s, descending=True, stable=True)
        k = min(nms_pre, s.numel()) if nms_pre > 0 else s.numel()
        out.append((order[:k].int(), ranked[:k]))
    return out


def _check_select(ops, maps, nms_pre, what):
    segs = ops.RPNSegments(maps, nms_pre)
    idx, score = ops.rpn_select(segs)
    want = _select_ref(ops, maps, nms_pre)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (sum(len(w[0]) for w in want),) == tuple(score.shape)
    for s, (wi, ws) in enumerate(want):
        r0 = segs.row0[s]
        assert segs.rows[s] == len(wi)
        gi, gs = idx[r0:r0 + len(wi)], score[r0:r0 + len(wi)]
        assert torch.equal(gi, wi), f'{what}, segment {s}: {int((gi != wi).sum())} of {len(wi)} indices differ'
        assert torch.equal(gs.view(torch.int32), ws.view(torch.int32)), f'{what}, segment {s}: the scores differ'
    return segs, idx, score


# ------------------------------------------------------------------------------------------------ selection
CHUNK = 4096
# (A, H * W): the sizes 1, 63, 64, 65, 1023, 1025, the chunk and its neighbours and 3 x 67 x 101, each with the largest of
# A = 15 / 3 / 1 that divides it, and the multiples of 3 and 15 on either side of the chunk
SELECT_SIZES = [(1, 1), (3, 21), (1, 64), (1, 65), (3, 341), (1, 1025), (15, 273), (3, 1365), (1, CHUNK), (1, CHUNK + 1),
                (3, 1366), (15, 274), (3, 67 * 101), (15, 23 * 59)]


def test_select_sizes_cover_the_chunk():
    from dynamask_amd import ops
    assert ops.RPN_SELECT_CHUNK == CHUNK
    sizes = {a * hw for a, hw in SELECT_SIZES}
    assert {1, 63, 64, 65, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * 67 * 101} <= sizes


@pytest.mark.parametrize('A,hw', SELECT_SIZES)
def test_select_is_the_stable_sort_of_the_sigmoid(A, hw):
    from dynamask_amd import ops
    n = A * hw
    for kind in ('normal', 'coarse'):
        m = _map(A, hw, seed=n + A, kind=kind)
        for nms_pre in sorted({1, max(n - 1, 1), n, n + 5, 0, -1}):
            segs, idx, score = _check_select(ops, [m], nms_pre, f'A={A} HW={hw} {kind} nms_pre={nms_pre}')
            if nms_pre == n and kind == 'normal':
                again = ops.rpn_select(segs)
                assert torch.equal(again[0], idx) and torch.equal(again[1], score), 'two identical calls differ'
                assert sorted(idx.cpu().tolist()) == list(range(n))


@pytest.mark.parametrize('nms_pre', [1000, 70, 0])
def test_select_of_several_unequal_segments(nms_pre):
    from dynamask_amd import ops
    shapes = [(3, 67 * 101), (1, CHUNK + 1), (3, 21), (1, 1), (15, 274), (1, 1025), (1, 64)]
    maps = [_map(A, hw, seed=100 + i, kind='coarse' if i % 2 else 'normal') for i, (A, hw) in enumerate(shapes)]
    for count in (3, 5, 7):
        segs, idx, score = _check_select(ops, maps[:count], nms_pre, f'{count} segments, nms_pre={nms_pre}')
        # a segment's rows do not depend on the other segments of the call
        alone = ops.rpn_select(ops.RPNSegments(maps[1:2], nms_pre))
        r0 = segs.row0[1]
        assert torch.equal(alone[0], idx[r0:r0 + segs.rows[1]]) and torch.equal(alone[1], score[r0:r0 + segs.rows[1]])
    # the maps of one [B, A, H, W] tensor, image after image, are segments as they lie
    batch = torch.randn(3, 3, 21, 33, generator=_g(7)).cuda()
    _check_select(ops, [batch[b] for b in range(3)], nms_pre, 'images of one tensor')


def test_select_ties():
    from dynamask_amd import ops
    n = 3 * 67 * 101
    const = torch.full((3, 67, 101), 0.75).cuda()
    for nms_pre in (1, 1000, CHUNK + 1, 0):
        segs, idx, _ = _check_select(ops, [const], nms_pre, f'constant map, nms_pre={nms_pre}')
        assert torch.equal(idx, torch.arange(segs.rows[0], dtype=torch.int32, device='cuda'))
    # saturated logits tie exactly: +-100 mixed with zeros, the cut inside the group of ones and inside the zeros' 0.5
    pick = torch.randint(0, 3, (3, 67, 101), generator=_g(3))
    sat = torch.tensor([-100.0, 0.0, 100.0])[pick].cuda()
    ones, halves = int((pick == 2).sum()), int((pick == 1).sum())
    assert min(ones, halves) > 1000
    for nms_pre in (ones // 2, ones, ones + 1, ones + halves // 2, ones + halves + 7, 0):
        segs, idx, score = _check_select(ops, [sat, const], nms_pre, f'saturated map, nms_pre={nms_pre}')
    top = ops.rpn_select(ops.RPNSegments([sat], ones + 1))[1]
    assert float(top[ones - 1]) == 1.0 and float(top[ones]) == 0.5
    # an empty segment among others, and nothing at all
    empty = torch.zeros(3, 0, 5).cuda()
    segs, idx, score = _check_select(ops, [const[:, :2].contiguous(), empty, sat[:, :3].contiguous()], 100, 'an empty segment')
    assert segs.rows == [100, 0, 100]
    segs, idx, score = _check_select(ops, [empty], 100, 'only an empty segment')
    assert idx.numel() == 0
    idx, score = ops.rpn_select(ops.RPNSegments([], 100))
    assert idx.numel() == 0 and score.numel() == 0


# ------------------------------------------------------------------------------------------------ decode
def _generators():
    from dynamask_amd.anchors import AnchorGenerator
    return {'fpn': AnchorGenerator(strides=[4, 8, 16, 32, 64], ratios=[0.5, 1.0, 2.0], scales=[8]),
            'c4': AnchorGenerator(strides=[16], ratios=[0.5, 1.0, 2.0], scales=[2, 4, 8, 16, 32])}


@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_decode_is_bbox_decode_on_materialised_anchors(form):
    from dynamask_amd import ops
    gen = _generators()[form]
    L = gen.num_levels
    sizes = [(max(1, -(-67 // s[1])), max(1, -(-101 // s[0]))) for s in gen.strides] if form == 'fpn' else [(13, 21)]
    shapes = [(67, 101, 3), (59, 90, 3)]
    B = len(shapes)
    table, base_rows = gen.base_anchor_table('cuda')
    anchors = gen.grid_anchors(sizes, device='cuda')
    img_tab = ops.image_shape_table([dict(img_shape=s) for s in shapes], 'cuda')
    clipped = beyond = 0
    for means, stds in (((0., 0., 0., 0.), (1., 1., 1., 1.)), ((0.1, -0.1, 0.05, 0.), (0.5, 0.5, 0.25, 0.25))):
        logits, deltas = [], []
        for b in range(B):
            for l, (h, w) in enumerate(sizes):
                A = gen.num_base_anchors[l]
                logits.append(torch.randn(A, h, w, generator=_g(10 * b + l)).cuda())
                d = 0.5 * torch.randn(4 * A, h, w, generator=_g(50 + 10 * b + l))
                far = torch.rand(d.shape, generator=_g(90 + 10 * b + l)) < 1 / 8
                deltas.append(torch.where(far, d * 12, d).cuda())
        for nms_pre in (0, 300):
            segs = ops.RPNSegments(logits, nms_pre, deltas, strides=[gen.strides[l] for _ in range(B) for l in range(L)],
                                   base_rows=[base_rows[l] for _ in range(B) for l in range(L)],
                                   images=[b for b in range(B) for _ in range(L)], num_levels=L)
            idx, _ = ops.rpn_select(segs)
            got = ops.rpn_decode(segs, idx, table, img_tab, means, stds)
            assert tuple(got.shape) == (segs.total_rows, 4)
            for s in range(B * L):
                b, l = divmod(s, L)
                sel = idx[segs.row0[s]:segs.row0[s] + segs.rows[s]].long()
                d = deltas[s].permute(1, 2, 0).reshape(-1, 4)[sel].contiguous()
                want, _ = ops.bbox_decode(anchors[l][sel].contiguous(), None, d, 1, means, stds, 16 / 1000, shapes[b][:2],
                                          class_agnostic=True)
                mine = got[segs.row0[s]:segs.row0[s] + segs.rows[s]]
                assert torch.equal(mine.view(torch.int32), want.view(torch.int32)), \
                    f'{form} image {b} level {l}: {int((mine != want).any(1).sum())} of {len(want)} boxes differ'
                clipped += int(((want[:, 2] == shapes[b][1]) | (want[:, 3] == shapes[b][0]) | (want[:, :2] == 0).any(1)).sum())
                beyond += int((d[:, 2:].abs() * max(stds[2:]) > 4.2).any(1).sum())
            assert torch.equal(ops.rpn_decode(segs, idx, table, img_tab, means, stds), got), 'two identical calls differ'
    assert clipped > 50 and beyond > 50
    # an index that is no candidate of its segment gives a zero box, not a read outside the maps
    bad = idx.clone()
    bad[0], bad[-1] = -1, 1 << 30
    out = ops.rpn_decode(segs, bad, table, img_tab, means, stds)
    assert float(out[0].abs().sum()) == 0 and float(out[-1].abs().sum()) == 0 and torch.equal(out[1:-1], got[1:-1])


# ------------------------------------------------------------------------------------------------ merge
def _merge_case(ops, rows, kept, nms_post, L, seed, levels_of_scores=None):
    """rows / kept: per segment (image-major).  Returns what dm_rpn_merge gives and what concatenate + stable sort gives."""
    g = _g(seed)
    S = len(rows)
    segs = ops.RPNSegments([torch.zeros(1, 1, n).cuda() for n in rows], 0, num_levels=L)
    assert segs.rows == list(rows)
    scores, keeps = [], []
    for n, k in zip(rows, kept):
        s = torch.rand(n, generator=g)
        if levels_of_scores:
            s = torch.round(s * levels_of_scores) / levels_of_scores          # equal scores, within and across levels
        scores.append(torch.sort(s, descending=True)[0])
        kp = torch.sort(torch.randperm(n, generator=g)[:k])[0].int() if n else torch.zeros(0, dtype=torch.int32)
        keeps.append(torch.cat([kp, torch.full((n - k,), -7, dtype=torch.int32)]))       # the tail is never read
    score = torch.cat(scores).cuda()
    keep = torch.cat(keeps).cuda()
    boxes = torch.randn(sum(rows), 4, generator=g).cuda()
    kept_t = torch.tensor(kept, dtype=torch.int32).cuda()
    out, counts = ops.rpn_merge(segs, keep, kept_t, boxes, score, nms_post)
    counts = counts.cpu().tolist()
    for b in range(S // L):
        sel = torch.cat([keep[segs.row0[s]:segs.row0[s] + kept[s]].long() + segs.row0[s] for s in range(b * L, (b + 1) * L)])
        dets = torch.cat([boxes[sel], score[sel][:, None]], 1)
        order = torch.sort(dets[:, 4], descending=True, stable=True)[1][:nms_post]
        want = dets[order]
        assert counts[b] == len(want) == min(nms_post, sum(kept[b * L:(b + 1) * L]))
        got = out[b, :counts[b]]
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), \
            f'image {b}: {int((got != want).any(1).sum())} of {len(want)} rows differ'
    return out, counts


def test_merge_is_concatenate_and_stable_sort():
    from dynamask_amd import ops
    # two images of three levels; image 1 has an empty level and a level that kept nothing
    rows = [700, 300, 40, 513, 0, 257]
    kept = [650, 120, 40, 400, 0, 0]
    for nms_post in (1000, 256, 1):
        _merge_case(ops, rows, kept, nms_post, 3, seed=nms_post)
        _merge_case(ops, rows, kept, nms_post, 3, seed=nms_post + 1, levels_of_scores=16)
    # one level supplies everything; nothing is kept at all
    _merge_case(ops, [100, 900, 100], [0, 900, 0], 500, 3, seed=5)
    _merge_case(ops, [100, 900, 100], [0, 0, 0], 500, 3, seed=6)
    # one level (the C4 form), five levels, all scores equal: the order is level, then rank
    _merge_case(ops, [1200, 1100], [1000, 7], 1000, 1, seed=7, levels_of_scores=4)
    out, counts = _merge_case(ops, [30, 20, 10, 5, 3], [30, 20, 10, 5, 3], 50, 5, seed=8, levels_of_scores=1)
    assert counts == [50]


# ------------------------------------------------------------------------------------------------ the head
@pytest.fixture(scope='module')
def rpn(golden_dir):
    """({form: RPNHead on the device with the fixture's seeded weights}, the fixture, its JSON, rpn_inputs)."""
    import rpn_inputs as ri
    from dynamask_amd import dense_heads, registry  # noqa: F401
    z = dict(np.load(os.path.join(golden_dir, 'g26_rpn.npz')))
    with open(os.path.join(golden_dir, 'g26_rpn_configs.json')) as f:
        cfgs = json.load(f)
    heads = {}
    for form in cfgs:
        cfg = registry._to_cfgdict(cfgs[form])
        rh = dict(cfg.model.rpn_head)
        rh.update(train_cfg=None, test_cfg=cfg.test_cfg.rpn)
        m = registry.build_head(rh)
        m.load_state_dict(ri.head_state({k: v.shape for k, v in m.state_dict().items()}, int(z['seed'])), strict=True)
        heads[form] = m.cuda().eval()
    return heads, z, cfgs, ri


@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_forward_against_the_reference(rpn, form):
    from dynamask_amd import conv_precision, ops
    heads, z, _, ri = rpn
    m = heads[form]
    x = [f.cuda() for f in ri.feats(m.in_channels, [s[0] for s in m.anchor_generator.strides])]
    with torch.no_grad():
        cls, reg = m(x)
        with conv_precision('bf16x3'):
            cls3, reg3 = m(x)
    assert len(cls) == len(reg) == m.anchor_generator.num_levels
    for l in range(len(cls)):
        for name, got, other in (('cls', cls[l], cls3[l]), ('reg', reg[l], reg3[l])):
            ref32 = z[f'{form}_{name}{l}']
            assert tuple(got.shape) == ref32.shape
            assert_close_via_f64(got, ref32, ri.unpack_f64(ref32, z[f'{form}_{name}{l}_err16']), f'{form} {name}{l}')
            assert torch.equal(got, other), f'{form} {name}{l}: the bf16x3 mode changed the RPN'
        # each output has the bits of its own ops.conv2d on exactly packed weights
        with torch.no_grad():
            h = ops.conv2d(x[l], ops.pack_conv_weight(m.rpn_conv.weight.detach()), m.rpn_conv.bias.detach(), m.feat_channels, 3,
                           relu=True)
            c = ops.conv2d(h, ops.pack_conv_weight(m.rpn_cls.weight.detach()), m.rpn_cls.bias.detach(), m.num_anchors, 1)
            r = ops.conv2d(h, ops.pack_conv_weight(m.rpn_reg.weight.detach()), m.rpn_reg.bias.detach(), 4 * m.num_anchors, 1)
        assert torch.equal(c, cls[l]) and torch.equal(r, reg[l])
    assert float(torch.cat([c.flatten() for c in cls]).std()) > 1.0          # the logits span several units


@pytest.mark.parametrize('W', [128, 129, 200, 337])
def test_forward_on_wide_maps(W):
    """rpn_conv leaves ops.conv2d (whole rows in LDS) for the any-width 3x3 kernel above CONV2D_3X3_MAX_WIDTH: both sides of
    the threshold, and a map wider than ops.conv2d takes, against float64."""
    import torch.nn.functional as F
    import rpn_inputs as ri
    from dynamask_amd import dense_heads
    assert dense_heads.CONV2D_3X3_MAX_WIDTH == 128
    m = dense_heads.RPNHead(16, feat_channels=24, anchor_generator=dict(type='AnchorGenerator', scales=[8], ratios=[0.5, 1.0, 2.0],
                                                                      strides=[4]))
    m.load_state_dict(ri.head_state({k: v.shape for k, v in m.state_dict().items()}, W), strict=True)
    x = torch.randn(2, 16, 5, W, generator=_g(W))
    ref = {}
    for dt in (torch.float32, torch.float64):
        sd = {k: v.detach().to(dt) for k, v in m.state_dict().items()}
        h = F.relu(F.conv2d(x.to(dt), sd['rpn_conv.weight'], sd['rpn_conv.bias'], padding=1))
        ref[dt] = (F.conv2d(h, sd['rpn_cls.weight'], sd['rpn_cls.bias']), F.conv2d(h, sd['rpn_reg.weight'], sd['rpn_reg.bias']))
    m = m.cuda().eval()
    with torch.no_grad():
        cls, reg = m([x.cuda()])
        one = m([x[1:].cuda()])
    assert tuple(cls[0].shape) == (2, 3, 5, W) and tuple(reg[0].shape) == (2, 12, 5, W)
    assert_close_via_f64(cls[0], ref[torch.float32][0], ref[torch.float64][0], f'cls at width {W}')
    assert_close_via_f64(reg[0], ref[torch.float32][1], ref[torch.float64][1], f'reg at width {W}')
    assert torch.equal(one[0][0], cls[0][1:]) and torch.equal(one[1][0], reg[0][1:]), 'an image\'s bits depend on the batch'


def _fixture_maps(rpn, form):
    heads, z, cfgs, ri = rpn
    m = heads[form]
    cls, reg = ri.synthetic_maps(m.anchor_generator.num_base_anchors, [s[0] for s in m.anchor_generator.strides], int(z['seed']))
    cfg = dict(m.test_cfg)
    cfg['nms_pre'] = cfgs[form]['get_bboxes_nms_pre']
    return m, [c.cuda() for c in cls], [r.cuda() for r in reg], cfg


@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_get_bboxes_against_the_reference(rpn, form):
    from dynamask_amd import dense_heads, ops
    _, z, _, ri = rpn
    m, cls, reg, cfg = _fixture_maps(rpn, form)
    metas = ri.img_metas()
    assert dense_heads.RPN_FUSED[0]
    got = m.get_bboxes(cls, reg, metas, cfg=cfg)
    assert len(got) == ri.BATCH
    sizes = [c.shape[-2] * c.shape[-1] * c.shape[1] for c in cls]
    assert any(n > cfg['nms_pre'] for n in sizes)
    assert form == 'c4' or any(n <= cfg['nms_pre'] for n in sizes)
    for b in range(ri.BATCH):
        ref32 = z[f'{form}_dets_b{b}']
        assert tuple(got[b].shape) == ref32.shape, f'image {b}: {len(got[b])} proposals, the reference has {len(ref32)}'
        # the order: row r is candidate cand[r] of level level[r] -- its score is the library's sigmoid of that logit
        level, cand = z[f'{form}_level_b{b}'], z[f'{form}_cand_b{b}']
        logit = torch.stack([cls[int(l)][b].permute(1, 2, 0).reshape(-1)[int(c)] for l, c in zip(level, cand)])
        want_score = ops.sigmoid(logit.contiguous())
        assert torch.equal(got[b][:, 4], want_score), \
            f'image {b}: {int((got[b][:, 4] != want_score).sum())} of {len(cand)} rows are another candidate than the reference\'s'
        ref64 = ri.unpack_f64(ref32, z[f'{form}_dets_err16_b{b}'])
        assert_close_via_f64(got[b][:, :4], ref32[:, :4], ref64[:, :4], f'{form} boxes of image {b}')
        assert_close_via_f64(got[b][:, 4], ref32[:, 4], ref64[:, 4], f'{form} scores of image {b}')
    # rescale is ignored, as in the reference
    again = m.get_bboxes(cls, reg, metas, cfg=cfg, rescale=True)
    assert all(torch.equal(a, g) for a, g in zip(again, got))


@pytest.mark.parametrize('form', ['fpn', 'c4'])
def test_fused_and_composed_paths_give_the_same_bits(rpn, form, monkeypatch):
    from dynamask_amd import dense_heads
    _, _, _, ri = rpn
    m, cls, reg, cfg = _fixture_maps(rpn, form)
    metas = ri.img_metas()
    for nms_pre, nms_post in ((cfg['nms_pre'], cfg['nms_post']), (0, 1000), (77, 50)):
        c = dict(cfg, nms_pre=nms_pre, nms_post=nms_post)
        fused = m.get_bboxes(cls, reg, metas, cfg=c)
        monkeypatch.setattr(dense_heads, 'RPN_FUSED', [False])
        composed = m.get_bboxes(cls, reg, metas, cfg=c)
        monkeypatch.setattr(dense_heads, 'RPN_FUSED', [True])
        for b in range(ri.BATCH):
            assert fused[b].shape == composed[b].shape and 0 < len(fused[b]) <= nms_post
            assert torch.equal(fused[b].view(torch.int32), composed[b].view(torch.int32)), \
                f'nms_pre={nms_pre}: image {b}: {int((fused[b] != composed[b]).any(1).sum())} rows differ'
            # B = 2 in one call equals two B = 1 calls
            alone = m.get_bboxes([x[b:b + 1] for x in cls], [x[b:b + 1] for x in reg], [metas[b]], cfg=c)
            assert len(alone) == 1 and torch.equal(alone[0], fused[b])


def test_get_bboxes_waits_once(rpn, monkeypatch):
    """One host wait per call, whatever B and L are: the copy of the per-image counts."""
    import bench
    _, _, _, ri = rpn
    metas = ri.img_metas()
    for form in ('fpn', 'c4'):
        m, cls, reg, cfg = _fixture_maps(rpn, form)
        m.get_bboxes(cls, reg, metas, cfg=cfg)
        both = bench.count_host_syncs(lambda: m.get_bboxes(cls, reg, metas, cfg=cfg))
        one = bench.count_host_syncs(lambda: m.get_bboxes([x[:1] for x in cls], [x[:1] for x in reg], metas[:1], cfg=cfg))
        assert both == one == 1, (form, both, one)
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, 'cpu', lambda self, *a, **k: (calls.append(tuple(self.shape)), real(self, *a, **k))[1])
    m, cls, reg, cfg = _fixture_maps(rpn, 'fpn')
    m.get_bboxes(cls, reg, metas, cfg=cfg)
    assert calls == [(ri.BATCH,)]


def test_chain_into_the_roi_head(rpn, golden_dir):
    """simple_test_rpn(x) is get_bboxes(*forward(x)), and StandardRoIHead.simple_test takes its output as it is."""
    import c4_inputs as ci
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, shared_heads  # noqa: F401
    heads, z, cfgs, ri = rpn
    cfg = registry._to_cfgdict(cfgs['c4'])
    rh = dict(cfg.model.rpn_head)
    rh.update(train_cfg=None, test_cfg=dict(cfg.test_cfg.rpn, nms_post=24))
    m = registry.build_head(rh)
    m.load_state_dict(heads['c4'].state_dict(), strict=True)
    m = m.cuda().eval()
    x = [f.cuda() for f in ci.c4_feats(batch=2)]
    metas = ci.img_metas() * 2
    with torch.no_grad():
        proposals = m.simple_test_rpn(x, metas)
        composed = m.get_bboxes(*m(x), metas)
    assert len(proposals) == 2
    for p, c in zip(proposals, composed):
        assert p.dim() == 2 and p.shape[1] == 5 and 0 < len(p) <= 24 and torch.equal(p, c)
        assert bool((p[:-1, 4] >= p[1:, 4]).all()) and bool((p[:, :4] >= 0).all())
        assert bool((p[:, 2] <= ci.IMG_W).all()) and bool((p[:, 3] <= ci.IMG_H).all())
    with open(os.path.join(golden_dir, 'g25_c4_configs.json')) as f:
        c4 = registry._to_cfgdict(json.load(f)['faster_c4'])
    rc = dict(c4.model.roi_head)
    rc.update(train_cfg=None, test_cfg=c4.test_cfg.rcnn)
    roi = registry.build_head(rc)
    state = ci.head_state({k: v.shape for k, v in roi.state_dict().items()}, 25)
    roi.load_state_dict(state, strict=False)
    roi = roi.cuda().eval()
    for b in range(2):
        res = roi.simple_test([f[b:b + 1] for f in x], [proposals[b]], [metas[b]])
        assert len(res) == 80 and all(r.shape[1] == 5 for r in res)
