"""Batched multi-image inference (DynaMaskRoIHead.batch_simple_test and the pieces under it) against the one-image
entry points, and the multi-image post-processing kernels (dm_nms_mask_segmented + dm_nms_reduce_segmented,
dm_paste_masks_multi, dm_paste_rle_multi) against the one-image kernels."""
import numpy as np
import pytest
import torch

from oracle import ref_ops

pytestmark = pytest.mark.gpu

H, W = 256, 320                      # the padded batch the FPN maps are made for
THR = 0.5
BAND = 1e-3                          # probability band around mask_thr_binary where B > 1 may flip a pixel
METAS = [
    dict(img_shape=(256, 320, 3), ori_shape=(256, 320, 3), scale_factor=1.0),
    dict(img_shape=(240, 300, 3), ori_shape=(160, 200, 3), scale_factor=np.array([1.5] * 4, dtype=np.float32)),
    dict(img_shape=(192, 256, 3), ori_shape=(384, 512, 3), scale_factor=0.5),
    dict(img_shape=(256, 288, 3), ori_shape=(341, 384, 3), scale_factor=np.array([0.75] * 4, dtype=np.float32)),
]
N_PROPS = (40, 25, 33, 18)


def _test_cfg(score_thr=0.0):
    from dynamask_amd.registry import ConfigDict
    return ConfigDict(score_thr=score_thr, nms=dict(type='nms', iou_threshold=0.5), max_per_img=100, mask_thr_binary=THR)


def _head(kind, score_thr=0.0):
    from dynamask_amd import bbox_heads, losses, mask_heads, registry, roi_extractors, roi_head, synth  # noqa: F401
    common = dict(bbox_roi_extractor=dict(type='SingleRoIExtractor', **synth.BBOX_ROI_EXTRACTOR_CFG),
                  bbox_head=dict(type='Shared2FCBBoxHead', **synth.BBOX_HEAD_CFG),
                  mask_roi_extractor=dict(type='SingleRoIExtractor', **synth.MASK_ROI_EXTRACTOR_CFG),
                  test_cfg=_test_cfg(score_thr))
    sd = {**synth.init_mask_pre_state(seed=6), **synth.init_bbox_head_state(seed=8)}
    if kind == 'dynamask':
        m = registry.build_head(dict(type='DynaMaskRoIHead', mask_head=dict(type='DynaMaskHead', **synth.MASK_HEAD_CFG),
                                     **common))
        sd.update(synth.init_dynamask_head_state(seed=5, test_mode=True))
    else:
        up = kind.split('-')[1]
        mcfg = dict(type='FCNMaskHead', **synth.FCN_HEAD_CFG)
        if up == 'carafe':
            mcfg['upsample_cfg'] = dict(type='carafe', scale_factor=2, up_kernel=5, up_group=1, encoder_kernel=3,
                                        encoder_dilation=1, compressed_channels=64)
        m = registry.build_head(dict(type='StandardRoIHead', mask_head=mcfg, **common))
        sd.update(synth.init_fcn_head_state(seed=7, upsample=up, test_mode=True))
    m.load_state_dict(sd, strict=True)
    return m.cuda().eval()


def _inputs(B, n_props=N_PROPS, seed=0, rescale=True):
    """B images of different img_shape / ori_shape / scale_factor.  rescale=False: float scale factors only (the
    one-image paste geometry takes an array [w, h, w, h] only with rescale=True, as mmdet 2.3's)."""
    from dynamask_amd import synth
    x = [f.cuda() for f in synth.make_fpn(B, H, W, 256, seed=seed)]
    props = []
    for b in range(B):
        h, w = METAS[b]['img_shape'][:2]
        props.append(synth.make_rois(1, n_props[b], h, w, seed=seed + 10 + b, max_size=160.0)[:, 1:].contiguous().cuda())
    metas = [dict(m) for m in METAS[:B]]
    if not rescale:
        for m in metas:
            if not isinstance(m['scale_factor'], float):
                m['scale_factor'] = float(m['scale_factor'][0])
    return x, props, metas


def _one(x, b):
    return [f[b:b + 1].contiguous() for f in x]


def _by_detection(segm, labels):
    """per-class lists -> one entry per detection, in detection order (class lists keep detection order)."""
    seen = {}
    out = []
    for c in labels:
        k = seen.get(c, 0)
        out.append(segm[c][k])
        seen[c] = k + 1
    return out


def _band(m, x1, dets, labels, meta, rescale):
    """Per detection: pixels whose per-image probability lies in [THR - BAND, THR + BAND) -- two pastes of the
    per-image logits at the band's edges."""
    from dynamask_amd import ops
    from dynamask_amd.mask_heads import FCNMaskHead
    from dynamask_amd.postprocess import _paste_geometry
    from dynamask_amd.roi_head import bbox2roi
    sf = meta['scale_factor']
    if rescale and not isinstance(sf, float):
        sf = torch.from_numpy(sf).to(dets.device)
    bx = dets[:, :4] * sf if rescale else dets
    if isinstance(m.mask_head, FCNMaskHead):          # (every RoI head is a StandardRoIHead)
        pred = m._mask_forward(x1, bbox2roi([bx]).contiguous())['mask_pred']
        pred, _ = m.mask_head._selected(pred, bx, labels)
    else:
        pred = m.simple_test_mask_logits(x1, bx, labels).clone()
    cb, h, w = _paste_geometry(bx, meta['ori_shape'], sf, rescale)
    lo = ops.paste_masks(pred, cb, h, w, THR - BAND, apply_sigmoid=True).cpu().numpy()
    hi = ops.paste_masks(pred, cb, h, w, THR + BAND, apply_sigmoid=True).cpu().numpy()
    return lo & ~hi, pred


def _bbox_equal(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert u.dtype == v.dtype and u.shape == v.shape and np.array_equal(u, v)


@pytest.mark.parametrize('kind', ['dynamask', 'fcn-carafe'])
@pytest.mark.parametrize('B', [1, 2, 4])
@pytest.mark.parametrize('rescale', [False, True])
def test_batch_simple_test_equals_per_image_calls(kind, B, rescale):
    m = _head(kind)
    x, props, metas = _inputs(B, rescale=rescale)
    with torch.no_grad():
        got_bits = m.batch_simple_test(x, props, metas, rescale=rescale, encode=False)
        got_rles = m.batch_simple_test(x, props, metas, rescale=rescale, encode=True)
        assert len(got_bits) == B and len(got_rles) == B
        flipped = band_px = total_px = 0
        for b in range(B):
            x1 = _one(x, b)
            ref_bits = m.simple_test(x1, [props[b]], [metas[b]], rescale=rescale, encode=False)
            ref_rles = m.simple_test(x1, [props[b]], [metas[b]], rescale=rescale, encode=True)
            # boxes, scores, labels: bit-identical whatever B is
            _bbox_equal(got_bits[b][0], ref_bits[0])
            _bbox_equal(got_rles[b][0], ref_bits[0])
            dets, labels = m.simple_test_bboxes(x1, [metas[b]], [props[b]], m.test_cfg, rescale=rescale)
            lab = labels.tolist()
            assert len(lab) > 0
            gb, rb = _by_detection(got_bits[b][1], lab), _by_detection(ref_bits[1], lab)
            gr, rr = _by_detection(got_rles[b][1], lab), _by_detection(ref_rles[1], lab)
            assert [len(c) for c in got_bits[b][1]] == [len(c) for c in ref_bits[1]]
            if B == 1:
                assert all(np.array_equal(u, v) and u.dtype == np.bool_ for u, v in zip(gb, rb))
                assert gr == rr
                continue
            band, _ = _band(m, x1, dets, labels, metas[b], rescale)
            for j, (u, v) in enumerate(zip(gb, rb)):
                assert u.shape == v.shape and u.dtype == np.bool_
                ne = u != v
                assert not (ne & ~band[j]).any(), f'image {b} det {j}: a pixel outside the threshold band differs'
                flipped += int(ne.sum())
                band_px += int(band[j].sum())
                total_px += ne.size
                # the RLE form is the encoding of the batched bitmap
                assert gr[j] == ref_ops.rle_encode(u.astype(np.uint8))
    if B > 1:
        print(f'{kind} B={B} rescale={rescale}: {flipped} flipped pixels, {band_px} in the +-{BAND} band, of {total_px}')
        assert flipped <= band_px and flipped <= max(64, 1e-4 * total_px)


@pytest.mark.parametrize('kind', ['dynamask', 'fcn-carafe'])
def test_batch_mask_logits_close_to_per_image(kind):
    """B = 4: the logits of one mask chain over all images against each image's own chain (1e-4, the gate of the
    per-image path against the oracle in test_path_gpu.py); B = 1 bit-identical."""
    from dynamask_amd.mask_heads import FCNMaskHead
    from dynamask_amd.roi_head import bbox2roi
    m = _head(kind)
    x, props, metas = _inputs(4)
    with torch.no_grad():
        dl = m.batch_simple_test_bboxes(x, metas, props, m.test_cfg)
        sfs = [mt['scale_factor'] for mt in metas]
        merged, offs = m.batch_simple_test_mask_logits(x, [d for d, _ in dl], [l for _, l in dl], sfs, rescale=True)
        merged = merged.clone()
        assert offs == [0] + list(np.cumsum([d.shape[0] for d, _ in dl]))
        for b, (d, l) in enumerate(dl):
            sf = sfs[b] if isinstance(sfs[b], float) else torch.from_numpy(sfs[b]).cuda()
            bx = d[:, :4] * sf
            if isinstance(m.mask_head, FCNMaskHead):
                ref = m._mask_forward(_one(x, b), bbox2roi([bx]).contiguous())['mask_pred']
            else:
                ref = m.simple_test_mask_logits(_one(x, b), bx, l)
            np.testing.assert_allclose(merged[offs[b]:offs[b + 1]].cpu().numpy(), ref.cpu().numpy(), atol=1e-4, rtol=1e-4)
            one, o1 = m.batch_simple_test_mask_logits(_one(x, b), [d], [l], [sfs[b]], rescale=True)
            assert o1 == [0, d.shape[0]] and torch.equal(one, ref)


def test_empty_images():
    """No proposals for one image; every detection below score_thr; all images empty."""
    m = _head('dynamask')
    x, props, metas = _inputs(3, rescale=False)
    props[1] = props[1][:0]
    with torch.no_grad():
        got = m.batch_simple_test(x, props, metas, encode=True)
        assert all(len(b) == 0 for b in got[1][0]) and all(len(s) == 0 for s in got[1][1])
        assert len(got[1][0]) == 80 and len(got[1][1]) == 80
        for b in (0, 2):
            ref = m.simple_test(_one(x, b), [props[b]], [metas[b]], encode=True)
            _bbox_equal(got[b][0], ref[0])
            assert got[b][1] == ref[1]
        # all images empty: no proposals anywhere, or everything below score_thr
        for p in ([q[:0] for q in props], props):
            mm = m if p is not props else _head('dynamask', score_thr=1.1)
            res = mm.batch_simple_test(x, p, metas, encode=False)
            ref = mm.simple_test(_one(x, 0), [props[0]], [metas[0]]) if p is props else None
            for bb, sg in res:
                assert len(bb) == 80 and all(a.shape == (0, 5) and a.dtype == np.float32 for a in bb)
                assert sg == [[] for _ in range(80)]
            if ref is not None:
                _bbox_equal(res[0][0], ref[0])
        dets = mm.batch_simple_test_bboxes(x, metas, props, mm.test_cfg)
        assert all(d.shape == (0, 5) and l.shape == (0,) for d, l in dets)
        z, offs = m.batch_simple_test_mask_logits(x, [d for d, _ in dets], [l for _, l in dets])
        assert z.shape == (0, 1, 112, 112) and offs == [0, 0, 0, 0]


def test_graphed_batch_matches_eager_and_keys_on_B():
    m = _head('dynamask')
    x4, props, metas = _inputs(4)
    with torch.no_grad():
        dl = m.batch_simple_test_bboxes(x4, metas, props, m.test_cfg)
        dets, labs = [d[:40] for d, _ in dl], [l[:40] for _, l in dl]
        x2, x3 = [f[:2].contiguous() for f in x4], [f[:3].contiguous() for f in x4]
        e2 = m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0].clone()
        e3 = m.batch_simple_test_mask_logits(x3, dets[:3], labs[:3])[0].clone()
        gl = m.enable_inference_graphs(True)
        g2 = m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0].clone()
        assert gl.captures == 1 and gl.replays == 1
        g3 = m.batch_simple_test_mask_logits(x3, dets[:3], labs[:3])[0].clone()
        assert gl.captures == 2, 'a graph of B = 2 must not serve B = 3'
        assert {k[:2] for k in gl._graphs} == {('batch', 2), ('batch', 3)}
        np.testing.assert_allclose(g2.cpu().numpy(), e2.cpu().numpy(), atol=1e-4, rtol=1e-4)
        np.testing.assert_allclose(g3.cpu().numpy(), e3.cpu().numpy(), atol=1e-4, rtol=1e-4)
        # fewer rows in the same bucket (70 of 80) (rows past them must be zeroed), then the first call again
        g2s = m.batch_simple_test_mask_logits(x2, [dets[0], dets[1][:30]], [labs[0], labs[1][:30]])[0].clone()
        assert torch.equal(m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0], g2) and gl.captures == 2
        m.enable_inference_graphs(False)
        assert torch.equal(m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0], e2)
        e2s = m.batch_simple_test_mask_logits(x2, [dets[0], dets[1][:30]], [labs[0], labs[1][:30]])[0]
        np.testing.assert_allclose(g2s.cpu().numpy(), e2s.cpu().numpy(), atol=1e-4, rtol=1e-4)
        gl = m.enable_inference_graphs(True)              # a fresh cache: captures again, same bits
        assert torch.equal(m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0], g2) and gl.captures == 1
        # totals above the largest batch bucket run eagerly
        gl.batch_buckets = (64,)
        assert torch.equal(m.batch_simple_test_mask_logits(x2, dets[:2], labs[:2])[0], e2) and gl.captures == 1
        # one-image calls keep their own graphs and keys
        m.simple_test_mask_logits(_one(x4, 0), dets[0], labs[0])
        assert gl.captures == 2 and sum(not isinstance(k[0], str) for k in gl._graphs) == 1
        m.enable_inference_graphs(False)


def test_host_syncs_do_not_grow_with_B(monkeypatch):
    import bench
    m = _head('dynamask')
    calls = [0]
    real = torch.cuda.Stream.synchronize

    def counting(self):
        calls[0] += 1
        return real(self)
    monkeypatch.setattr(torch.cuda.Stream, 'synchronize', counting)
    for encode in (True, False):
        seen = {}
        for B in (1, 2, 4):
            x, props, metas = _inputs(B, rescale=False)
            with torch.no_grad():
                m.batch_simple_test(x, props, metas, encode=encode)        # warm
                torch.cuda.synchronize()
                calls[0] = 0
                n = bench.count_host_syncs(lambda: m.batch_simple_test(x, props, metas, encode=encode))
            assert n is not None
            seen[B] = n + calls[0]
        print('host syncs per batched call', 'encode' if encode else 'bitmaps', seen)
        assert len(set(seen.values())) == 1, seen


# ----------------------------------------------------------------------------- kernels against the one-image forms
def _seg_boxes(M, g):
    ctr = torch.rand(M, 2, generator=g) * 120
    wh = torch.rand(M, 2, generator=g) * 60 + 4
    return torch.cat([ctr - wh / 2, ctr + wh / 2], 1)


@pytest.mark.parametrize('offset', [0, 1])
def test_nms_segmented_matches_per_segment_nms(offset):
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(7)
    counts = [0, 1, 63, 64, 65, 150, 0, 7, 200]
    boxes, scores = [], []
    for M in counts:
        boxes.append(_seg_boxes(M, g))
        scores.append((torch.rand(M, generator=g) * 10).floor() / 10)     # ties in score
    sorted_boxes = []
    for bx, sc in zip(boxes, scores):
        o = torch.sort(sc, descending=True, stable=True)[1]
        sorted_boxes.append((bx[o], sc[o]))
    sb = torch.cat([b for b, _ in sorted_boxes]).cuda().contiguous()
    for max_num in (-1, 5, 64):
        keep, kept = ops.nms_segmented(sb, counts, 0.5, offset=offset, max_num=max_num)
        keep, kept = keep.cpu(), kept.cpu().tolist()
        start = 0
        for M, (bx, sc) in zip(counts, sorted_boxes):
            _, ref = ops.nms(bx.cuda().contiguous(), sc.cuda().contiguous(), 0.5, offset=offset, max_num=max_num)
            ref = ref.cpu().tolist()
            got = keep[start:start + len(ref)].tolist()
            assert got == ref, (M, max_num)
            start += M
        assert kept == [len(ops.nms(bx.cuda().contiguous(), sc.cuda().contiguous(), 0.5, offset=offset,
                                    max_num=max_num)[1]) for bx, sc in sorted_boxes]


def test_multiclass_nms_batch_matches_per_image():
    from dynamask_amd.postprocess import multiclass_nms, multiclass_nms_batch
    g = torch.Generator().manual_seed(11)
    rows = [0, 5, 37, 120, 9]
    bl, sl = [], []
    for i, n in enumerate(rows):
        base = _seg_boxes(n, g) * (1 + i)                    # a different largest coordinate per image
        bl.append((base[:, None, :] + torch.randn(n, 80, 4, generator=g)).reshape(n, 320).cuda())
        s = torch.softmax(torch.randn(n, 81, generator=g) * 3, 1)
        if i == 4:
            s = s * 0.01                                    # every candidate below score_thr
        sl.append(s.cuda())
    for max_num in (100, 10, -1):
        got = multiclass_nms_batch(bl, sl, 0.05, dict(type='nms', iou_threshold=0.5), max_num)
        for b in range(len(rows)):
            rd, rl = multiclass_nms(bl[b], sl[b], 0.05, dict(type='nms', iou_threshold=0.5), max_num)
            assert torch.equal(got[b][0], rd) and torch.equal(got[b][1], rl), (b, max_num)
        assert got[0][0].shape == (0, 5) and got[4][0].shape == (0, 5)
        assert all(d.shape[0] > 0 for d, _ in got[1:4])
    agn = multiclass_nms_batch(bl, sl, 0.05, dict(type='nms', iou_threshold=0.5, class_agnostic=True), 100)
    for b in range(len(rows)):
        rd, rl = multiclass_nms(bl[b], sl[b], 0.05, dict(type='nms', iou_threshold=0.5, class_agnostic=True), 100)
        assert torch.equal(agn[b][0], rd) and torch.equal(agn[b][1], rl)


def test_paste_multi_matches_single_image_kernels():
    from dynamask_amd import ops
    g = torch.Generator().manual_seed(13)
    sizes = [(1, 1), (5, 4000), (120, 90), (64, 64), (33, 17)]
    counts = [2, 3, 0, 4, 1]
    masks, boxes = [], []
    for (h, w), n in zip(sizes, counts):
        masks.append(torch.randn(n, 1, 28, 28, generator=g) * 3)
        x1 = torch.rand(n, generator=g) * w * 1.4 - 0.2 * w           # some boxes outside the canvas
        y1 = torch.rand(n, generator=g) * h * 1.4 - 0.2 * h
        bw = torch.rand(n, generator=g) * w + 0.5
        bh = torch.rand(n, generator=g) * h + 0.5
        boxes.append(torch.stack([x1, y1, x1 + bw, y1 + bh], 1))
    M = torch.cat(masks).cuda().contiguous()
    Bx = torch.cat(boxes).cuda().contiguous()
    for sig in (True, False):
        thr = THR if sig else 0.0
        buf, offs, det_sizes = ops.paste_masks_multi(M, Bx, counts, sizes, thr, apply_sigmoid=sig)
        rles = ops.paste_rle_multi(M, Bx, counts, sizes, thr, apply_sigmoid=sig)
        short = ops.paste_rle_multi(M, Bx, counts, sizes, thr, apply_sigmoid=sig, capacity=1)   # overflow + re-run
        flat = buf.cpu().numpy()
        assert buf.numel() == sum(n * h * w for (h, w), n in zip(sizes, counts))
        n0 = 0
        for (h, w), n in zip(sizes, counts):
            if n == 0:
                continue
            ref = ops.paste_masks(M[n0:n0 + n], Bx[n0:n0 + n], h, w, thr, apply_sigmoid=sig).cpu().numpy()
            ref_rle = ops.paste_rle(M[n0:n0 + n], Bx[n0:n0 + n], h, w, thr, apply_sigmoid=sig)
            for k in range(n):
                j = n0 + k
                assert det_sizes[j] == (h, w)
                got = flat[offs[j]:offs[j] + h * w].reshape(h, w).astype(bool)
                assert np.array_equal(got, ref[k]), (h, w, k, sig)
                assert rles[j] == ref_rle[k] == short[j]
            n0 += n
    assert ops.paste_rle_multi(M[:0], Bx[:0], [0, 0], [(3, 3), (4, 4)]) == []
