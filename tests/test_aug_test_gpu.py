"""Test-time augmentation (DynaMaskRoIHead.aug_test and the pieces under it) on the device: the three kernels
(dm_bbox_mapping_multi, dm_merge_aug_bboxes, dm_merge_aug_masks) against torch restatements, StandardRoIHead.aug_test
against the reference's own aug_test (g16), the degenerate augmentations against simple_test bit for bit, the DynaMask
definition against a composition of public calls, and graphs against eager."""
import os

import numpy as np
import pytest
import torch

import aug_inputs as ai
from oracle import ref_ops

pytestmark = pytest.mark.gpu

THR = 0.5
BAND = 1e-3


def _cfg(score_thr=0.05):
    from dynamask_amd.registry import ConfigDict
    return ConfigDict(score_thr=score_thr, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=THR)


def _head(kind, score_thr=0.05):
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    common = dict(bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
                  bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
                  mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
                  test_cfg=_cfg(score_thr))
    if kind == 'dynamask':
        m = registry.build_head(dict(type='DynaMaskRoIHead', mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG),
                                     **common))
        sd = {**synth.init_mask_pre_state(seed=6), **synth.init_bbox_head_state(seed=8),
              **synth.init_dynamask_head_state(seed=5, test_mode=True)}
    else:
        m = registry.build_head(dict(type='StandardRoIHead', mask_head=dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG),
                                     **common))
        sd = ai.head_state()
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _case(case):
    x, props, metas = ai.case_inputs(case)
    return [[t.cuda() for t in xv] for xv in x], props.cuda(), metas


def _view_rows(views):
    """(sf fp32 [4], img_h, img_w, flip direction or None) per view, from (scale_factor, img_shape, direction)."""
    out = []
    for sf, (h, w), d in views:
        s = np.asarray(sf, np.float32).reshape(-1)
        out.append((np.repeat(s, 4) if s.size == 1 else s, h, w, d))
    return out


def _metas(views):
    return [dict(img_shape=(h, w, 3), scale_factor=sf, flip=d is not None, flip_direction=d) for sf, (h, w), d in views]


def _torch_flip(b, h, w, d):
    """bbox_flip (core/bbox/transforms.py:5-27) on [n, 4k]."""
    f = b.clone()
    if d == 'horizontal':
        f[:, 0::4] = w - b[:, 2::4]
        f[:, 2::4] = w - b[:, 0::4]
    elif d == 'vertical':
        f[:, 1::4] = h - b[:, 3::4]
        f[:, 3::4] = h - b[:, 1::4]
    return f


def _torch_mapping(boxes, rows):
    out = []
    for s, h, w, d in rows:
        b = boxes[:, :4] * torch.from_numpy(s).to(boxes.device)
        b = _torch_flip(b, h, w, d)
        out.append(torch.cat([b.new_zeros((b.shape[0], 1)), b], 1))
    return torch.stack(out)


def _torch_merge_bboxes(bl, sl, rows):
    acc_b = acc_s = None
    for b, sc, (s, h, w, d) in zip(bl, sl, rows):
        r = _torch_flip(b, h, w, d)
        r = (r.view(-1, 4) / torch.from_numpy(s).to(b.device)).view(b.shape)
        acc_b = r if acc_b is None else acc_b + r
        acc_s = sc if acc_s is None else acc_s + sc
    return acc_b / len(bl), acc_s / len(bl)


VIEWS = [(1.0, (120, 160), None), (np.array([1.5, 1.25, 1.5, 1.25], np.float32), (150, 240), 'horizontal'),
         (0.75, (90, 120), 'vertical'), (1.25, (150, 200), 'horizontal'), (2.0, (240, 320), None),
         (0.5, (60, 80), 'vertical'), (1.0, (120, 160), 'horizontal'), (1.5, (180, 240), None)]


@pytest.mark.parametrize('V', [1, 3, 8])
def test_bbox_mapping_multi_equals_torch_bits(V):
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(V)
    boxes = torch.rand(57, 5, generator=g) * 150
    boxes[:, 2:4] += boxes[:, 0:2]
    boxes = boxes.cuda()
    views = VIEWS[:V]
    tab = ops.aug_view_table(_metas(views), boxes.device)
    got = ops.bbox_mapping_multi(boxes, tab)
    ref = _torch_mapping(boxes, _view_rows(views))
    assert got.shape == (V, 57, 5)
    assert torch.equal(got, ref)
    assert torch.equal(got.cpu(), _torch_mapping(boxes.cpu(), _view_rows(views)))
    # a [n, 4] input and a strided [n, 4] view of [n, 5] map alike
    assert torch.equal(ops.bbox_mapping_multi(boxes[:, :4].contiguous(), tab), got)
    assert torch.equal(ops.bbox_mapping_multi(boxes[:, 1:], tab), _torch_mapping(boxes[:, 1:], _view_rows(views)))


@pytest.mark.parametrize('V', [1, 2, 8])
def test_merge_aug_bboxes_equals_torch_bits(V):
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(10 + V)
    n, C = 45, 80
    bl = [(torch.rand(n, 4 * C, generator=g) * 200).cuda() for _ in range(V)]
    sl = [torch.softmax(torch.randn(n, C + 1, generator=g) * 3, 1).cuda() for _ in range(V)]
    views = VIEWS[:V]
    tab = ops.aug_view_table(_metas(views), bl[0].device)
    gb, gs = ops.merge_aug_bboxes(bl, sl, tab)
    rb, rs = _torch_merge_bboxes(bl, sl, _view_rows(views))
    assert torch.equal(gb, rb) and torch.equal(gs, rs)
    cb, cs = _torch_merge_bboxes([b.cpu() for b in bl], [s.cpu() for s in sl], _view_rows(views))
    assert torch.equal(gb.cpu(), cb) and torch.equal(gs.cpu(), cs)


def _f64_merge_masks(logits, labels, dirs):
    acc = 0
    for L, d in zip(logits, dirs):
        L = L.double().cpu()
        sel = L[torch.arange(L.shape[0]), labels.cpu() if L.shape[1] > 1 else 0][:, None]
        p = torch.sigmoid(sel)
        if d == 'horizontal':
            p = torch.flip(p, [3])
        elif d == 'vertical':
            p = torch.flip(p, [2])
        acc = acc + p
    return acc / len(logits)


@pytest.mark.parametrize('K,S,V', [(1, 112, 4), (5, 28, 3), (80, 28, 8), (1, 13, 1)])
def test_merge_aug_masks_against_f64(K, S, V):
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(K * 100 + S + V)
    n = 23
    logits = [(torch.randn(n, K, S, S, generator=g) * 4).cuda() for _ in range(V)]
    labels = torch.randint(0, K, (n,), generator=g).cuda()
    views = VIEWS[:V]
    tab = ops.aug_view_table(_metas(views), labels.device)
    got = ops.merge_aug_masks(logits, labels, tab)
    assert got.shape == (n, 1, S, S)
    ref = _f64_merge_masks(logits, labels, [d for _, _, d in views])
    assert (got.double().cpu() - ref).abs().max().item() < 1e-6
    if K > 1:        # the class channel: a merge of the pre-selected channel gives the same bits
        sel = [L[torch.arange(n, device=L.device), labels][:, None].contiguous() for L in logits]
        assert torch.equal(ops.merge_aug_masks(sel, None, tab), got)


@pytest.mark.parametrize('direction', ['horizontal', 'vertical'])
def test_merge_aug_masks_of_a_mirrored_pair_is_exact(direction):
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(7)
    L = (torch.randn(9, 1, 112, 112, generator=g) * 3).cuda()
    mirrored = torch.flip(L, [3 if direction == 'horizontal' else 2]).contiguous()
    one = ops.merge_aug_masks([L], None, ops.aug_view_table(_metas([(1.0, (10, 10), None)]), L.device))
    pair = ops.merge_aug_masks([L, mirrored], None,
                               ops.aug_view_table(_metas([(1.0, (10, 10), None), (1.0, (10, 10), direction)]), L.device))
    assert torch.equal(pair, one)
    # one view: the probabilities the paste itself computes from the logits (same sigmoid) -> same bitmaps
    boxes = (torch.rand(9, 4, generator=g) * 60).cuda()
    boxes[:, 2:] += boxes[:, :2] + 4
    a = ops.paste_masks(L, boxes, 80, 90, THR, apply_sigmoid=True)
    b = ops.paste_masks(one, boxes, 80, 90, THR, apply_sigmoid=False)
    assert torch.equal(a, b)


def _by_detection(segm, labels):
    seen, out = {}, []
    for c in labels:
        k = seen.get(c, 0)
        out.append(segm[c][k])
        seen[c] = k + 1
    return out


def _band(probs, boxes, h, w):
    from dynamask_amd import ops
    lo = ops.paste_masks(probs, boxes, h, w, THR - BAND, apply_sigmoid=False).cpu().numpy()
    hi = ops.paste_masks(probs, boxes, h, w, THR + BAND, apply_sigmoid=False).cpu().numpy()
    return lo & ~hi


@pytest.mark.parametrize('case', list(ai.CASES))
def test_fcn_aug_test_matches_reference_golden(golden_dir, case):
    """StandardRoIHead.aug_test (FCNMaskHead, deconv) against g16 = the reference's own aug_test on the CPU."""
    g = np.load(os.path.join(golden_dir, 'g16_aug.npz'))
    m = _head('fcn')
    x, props, metas = _case(case)
    with torch.no_grad():
        dets, labels = m.aug_test_bboxes(x, metas, [props], m.test_cfg)
        probs = m.aug_test_mask_probs(x, metas, dets, labels)
        bbox_results, segm_results = m.aug_test(x, [props], metas, rescale=True)
    lab = labels.cpu().numpy()
    assert np.array_equal(lab, g[f'{case}_labels'])
    np.testing.assert_allclose(dets.cpu().numpy(), g[f'{case}_dets'], rtol=1e-5, atol=1e-4)
    assert [len(b) for b in bbox_results] == g[f'{case}_bbox_counts'].tolist()
    np.testing.assert_allclose(np.concatenate([b for b in bbox_results if len(b)]),
                               np.concatenate([g[f'{case}_dets'][lab == c] for c in range(80) if (lab == c).any()]),
                               rtol=1e-5, atol=1e-4)
    gp = g[f'{case}_probs']
    assert probs.shape == (len(lab), 1, 28, 28)
    assert np.abs(probs[:, 0].cpu().numpy() - gp).max() < 1e-5
    h, w = ai.ORI_SHAPE[:2]
    band = _band(torch.from_numpy(gp)[:, None].contiguous().cuda(), dets[:, :4].contiguous(), h, w)
    bits = np.stack(_by_detection(segm_results, lab.tolist()))
    assert bits.dtype == np.bool_ and bits.shape == g[f'{case}_bits'].shape
    ne = bits != g[f'{case}_bits'].astype(bool)
    print(f'{case}: {int(ne.sum())} pixels differ from the golden, {int(band.sum())} in the band')
    assert not (ne & ~band).any()


def _single_view_inputs():
    from dynamask_amd import synth
    x = [f.cuda() for f in synth.make_fpn(1, 200, 256, 256, seed=21)]
    props = synth.make_rois(1, 40, 200, 256, seed=22, max_size=150.0)[:, 1:].contiguous().cuda()
    meta = dict(img_shape=(200, 256, 3), ori_shape=(200, 256, 3), scale_factor=1.0, flip=False, flip_direction=None)
    return x, props, meta


@pytest.mark.parametrize('kind', ['dynamask', 'fcn'])
@pytest.mark.parametrize('V', [1, 2])
@pytest.mark.parametrize('encode', [False, True])
def test_degenerate_augmentation_equals_simple_test(kind, V, encode):
    """One view at scale 1.0 without a flip, or V identical ones ((a + a) / 2 = a): simple_test(rescale=True), bit for
    bit -- boxes, scores, labels and masks (encode: the same RLE)."""
    m = _head(kind, score_thr=0.0)
    x, props, meta = _single_view_inputs()
    with torch.no_grad():
        ref_b, ref_s = m.simple_test(x, [props], [meta], rescale=True, encode=encode)
        got_b, got_s = m.aug_test([x] * V, [props], [[meta]] * V, rescale=True, encode=encode)
    assert len(got_b) == len(ref_b) and sum(len(b) for b in ref_b) > 0
    for u, v in zip(got_b, ref_b):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)
    assert [len(c) for c in got_s] == [len(c) for c in ref_s]
    for cu, cv in zip(got_s, ref_s):
        for u, v in zip(cu, cv):
            if encode:
                assert u == v
            else:
                assert u.dtype == np.bool_ and np.array_equal(u, v)


def test_aug_test_rescale_false_scales_only_the_boxes():
    m = _head('fcn')
    x, props, metas = _case('ms')
    with torch.no_grad():
        b1, s1 = m.aug_test(x, [props], metas, rescale=True)
        b0, s0 = m.aug_test(x, [props], metas, rescale=False)
    sf = torch.from_numpy(metas[0][0]['scale_factor'])
    for u, v in zip(b0, b1):
        ref = torch.from_numpy(v.copy())
        ref[:, :4] *= sf
        assert np.array_equal(u, ref.numpy())
    for cu, cv in zip(s0, s1):
        assert all(np.array_equal(u, v) for u, v in zip(cu, cv))


def test_dynamask_aug_test_against_public_composition():
    """The DynaMask definition at V = 4 (two scales x flip): per-view simple_test_mask_logits on the mapped boxes, torch
    sigmoid, flip back, mean, ops.paste_masks(apply_sigmoid=False)."""
    from dynamask_amd import ops
    m = _head('dynamask')
    x, props, metas = _case('ms')
    views = [mm[0] for mm in metas]
    with torch.no_grad():
        dets, labels = m.aug_test_bboxes(x, metas, [props], m.test_cfg)
        assert dets.shape[0] > 0
        probs = m.aug_test_mask_probs(x, metas, dets, labels)
        _, segm = m.aug_test(x, [props], metas, rescale=True)
        rows = _view_rows([(v['scale_factor'], v['img_shape'][:2], v['flip_direction'] if v['flip'] else None)
                           for v in views])
        mapped = _torch_mapping(dets, rows)
        ps = []
        for v, meta in enumerate(views):
            p = torch.sigmoid(m.simple_test_mask_logits(x[v], mapped[v][:, 1:], labels).clone())
            if meta['flip']:
                p = torch.flip(p, [3] if meta['flip_direction'] == 'horizontal' else [2])
            ps.append(p)
        ref = torch.stack(ps).mean(0).contiguous()
    assert probs.shape == ref.shape == (dets.shape[0], 1, 112, 112)
    assert (probs - ref).abs().max().item() < 1e-5
    h, w = ai.ORI_SHAPE[:2]
    boxes = dets[:, :4].contiguous()
    want = ops.paste_masks(ref, boxes, h, w, THR, apply_sigmoid=False).cpu().numpy()
    band = _band(ref, boxes, h, w)
    got = np.stack(_by_detection(segm, labels.tolist()))
    assert not ((got != want) & ~band).any()


def test_graphed_views_equal_eager():
    """Graphs on, two views of the same maps (one flipped): both replay ONE graph, whose static output the second
    replay overwrites -- the result must still equal the eager one."""
    m = _head('dynamask')
    x, props, metas = _case('ms')
    xs, ms = [x[0], x[0]], [metas[0], metas[1]]
    with torch.no_grad():
        m.enable_inference_graphs(False)
        eager = m.aug_test(xs, [props], ms, rescale=True)
        dets, labels = m.aug_test_bboxes(xs, ms, [props], m.test_cfg)
        p_eager = m.aug_test_mask_probs(xs, ms, dets, labels)
        graphs = m.enable_inference_graphs(True)
        try:
            graphed = m.aug_test(xs, [props], ms, rescale=True)
            p_graphed = m.aug_test_mask_probs(xs, ms, dets, labels)
            assert graphs.replays >= 4
        finally:
            m.enable_inference_graphs(False)
    assert torch.equal(p_eager, p_graphed)
    for u, v in zip(eager[0], graphed[0]):
        assert np.array_equal(u, v)
    for cu, cv in zip(eager[1], graphed[1]):
        assert all(np.array_equal(u, v) for u, v in zip(cu, cv))


@pytest.mark.parametrize('kind', ['dynamask', 'fcn'])
def test_aug_encode_gives_the_rle_of_the_bitmaps(kind):
    m = _head(kind)
    x, props, metas = _case('vf')
    with torch.no_grad():
        _, bits = m.aug_test(x, [props], metas, rescale=True)
        _, rles = m.aug_test(x, [props], metas, rescale=True, encode=True)
    assert [len(c) for c in bits] == [len(c) for c in rles] and sum(len(c) for c in bits) > 0
    for cb, cr in zip(bits, rles):
        for b, r in zip(cb, cr):
            assert r == ref_ops.rle_encode(b.astype(np.uint8))


class _Counting:
    def __init__(self, real):
        self._real, self.calls = real, 0

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith('dm_'):
            return fn

        def counted(*a):
            self.calls += 1
            return fn(*a)
        return counted


def _count_library_calls(fn):
    from dynamask_amd import _lib
    _lib.lib()
    real = _lib._LIB
    proxy = _Counting(real)
    _lib._LIB = proxy
    try:
        fn()
    finally:
        _lib._LIB = real
    return proxy.calls


@pytest.mark.parametrize('kind', ['dynamask', 'fcn'])
def test_aug_edge_cases(kind):
    m = _head(kind, score_thr=1.1)                       # no candidate survives the score cut
    x, props, metas = _case('ms')
    with torch.no_grad():
        bbox_results, segm = m.aug_test(x, [props], metas)
        assert all(b.shape == (0, 5) for b in bbox_results) and segm == [[] for _ in range(80)]
        empty = torch.zeros((0, 5), device='cuda')
        nolab = torch.zeros((0,), device='cuda', dtype=torch.long)
        assert _count_library_calls(lambda: m.aug_test_mask(x, metas, empty, nolab)) == 0
        bad = [[dict(mm[0])] for mm in metas]
        bad[2][0]['flip'], bad[2][0]['flip_direction'] = True, 'sideways'
        dets = torch.tensor([[10., 10., 50., 60., 0.9]], device='cuda')
        lab = torch.zeros((1,), device='cuda', dtype=torch.long)
        raised = []

        def attempt(call):
            try:
                call()
            except ValueError:
                raised.append(1)
        for call in (lambda: m.aug_test(x, [props], bad), lambda: m.aug_test_mask(x, bad, dets, lab),
                     lambda: m.aug_test(x[:3], [props], metas), lambda: m.aug_test_mask_probs(x, metas[:2], dets, lab)):
            assert _count_library_calls(lambda: attempt(call)) == 0       # raised before any launch
        assert len(raised) == 4


def test_aug_host_waits_do_not_grow_with_views():
    import bench
    m = _head('dynamask')
    x, props, metas = _case('ms')
    with torch.no_grad():
        m.aug_test(x, [props], metas)
        n2 = bench.count_host_syncs(lambda: m.aug_test(x[:2], [props], metas[:2]))
        n4 = bench.count_host_syncs(lambda: m.aug_test(x, [props], metas))
    assert n2 is not None and n2 == n4, (n2, n4)
