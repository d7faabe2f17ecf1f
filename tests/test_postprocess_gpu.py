"""The five kernels every RoI head ends in, each against an exact or float64 restatement of its operation (csrc/bbox.hip,
csrc/pointwise.hip, csrc/rle.hip): dm_bbox_decode and dm_cascade_refine against delta2bbox / softmax in float64 through
the triangle of tests/tolerances.py; the NMS suppression matrix bit by bit against the float64 IoU and the two greedy
passes against a Python walk over synthetic bit matrices; the paste against a float64 grid_sample, pixel by pixel
outside a band worked out from the fp32 reference's own error; the RLE encoder against the integer-exact oracle at the
joints of its 16 / 1024 / 4096-pixel units.  Where the library is called directly the outputs lie between canary bands
that must survive."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model, ref_ops
from tolerances import assert_close_via_f64
from test_postprocess_cpu import greedy_walk, max_keeps, pack_rows, random_upper_bits

pytestmark = pytest.mark.gpu

GUARD = 1024
OK = 0
ULP = 2.0 ** -23


def _lib():
    from dynamask_amd._lib import lib
    return lib()


class Guarded:
    """A device tensor of ``shape`` and ``dtype`` between two guard bands of ``canary`` (the tensor starts as canary too)."""

    def __init__(self, shape, dtype, canary):
        n = int(np.prod(shape))
        self.canary = canary
        self.buf = torch.full((n + 2 * GUARD,), canary, device='cuda', dtype=dtype)
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == self.canary).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == self.canary).all()), f'{what}: the guard band past the output was overwritten'


def _dev(t):
    return t.contiguous().cuda()


# ================================================================================================ 1. bbox_decode
MEANS, STDS = (0.01, -0.02, 0.03, 0.05), (0.1, 0.1, 0.2, 0.2)
CLIP = (97, 131)                       # max_shape (h, w)
WH_RATIO_CLIP = 16 / 1000


def _decode_inputs(N, NC, agnostic, seed):
    """Random RoIs, logits and deltas with the planted rows, plant k in row k where the case has that many rows.  Boxes:
    dw and dh above the clip, below it, an RoI of zero size.  Logits: spread over +-80, -inf entries, all equal, the
    maximum in a column of the second wave with -80 everywhere else."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(N, 2, generator=g) * 100
    wh = torch.rand(N, 2, generator=g) * 59 + 1
    boxes = torch.cat([xy, xy + wh], 1)
    cls = torch.randn(N, NC + 1, generator=g) * 3
    pred = torch.randn(N, 4 * (1 if agnostic else NC), generator=g)
    big = 40.0                                                # 40 * 0.2 = 8 > |log(16 / 1000)| = 4.135
    if N > 0:
        pred.view(N, -1, 4)[0, :, 2:] = big
    if N > 1:
        pred.view(N, -1, 4)[1, :, 2:] = -big
    if N > 2:
        boxes[2, 2:] = boxes[2, :2]
    if N > 0:
        cls[0] = torch.linspace(-80, 80, NC + 1)[torch.randperm(NC + 1, generator=g)]
    if N > 1:
        cls[1] = float('-inf')
        cls[1, NC] = 0.7
        cls[1, NC // 2] = -1.3
    if N > 2:
        cls[2] = 1.25
    if N > 3:
        cls[3] = -80.0                                        # columns 64..127 belong to the second wave
        cls[3, min(64, NC)] = 80.0
    return boxes, cls, pred


def _rois_of(boxes, width):
    if width == 4:
        return boxes.clone()
    col = (torch.arange(boxes.shape[0]) % 3).to(boxes.dtype)
    return torch.cat([col[:, None], boxes], 1)


def _ref_get_bboxes(boxes, cls, pred, max_shape, scale, means, stds, dtype):
    rois = torch.cat([boxes.new_zeros(boxes.shape[0], 1), boxes], 1).to(dtype)
    sf = (scale[0], scale[1], scale[0], scale[1])
    return ref_model.get_bboxes(rois, None if cls is None else cls.to(dtype), None if pred is None else pred.to(dtype),
                                max_shape, sf, rescale=True, means=means, stds=stds)


def _softmax_ulps(n):
    """fp32 error of one softmax entry, in units of 2^-23 relative, with the kernel's summation restated: expf twice
    (numerator, denominator: 2 each), the subtraction s - m (half an ulp of s - m, i.e. (m - s) / 2 ulps of the
    exponential; weighted by the entry's own probability that is at most log(n) / 2 in the row sum, on both sides),
    ceil(n / 128) + 7 additions of half an ulp, one division."""
    return 2 + 2 + math.log(max(n, 2)) + (math.ceil(n / 128) + 7) / 2 + 0.5


def _check_scores(got, cls, what):
    n = cls.shape[1]
    got64 = got.double()
    assert bool(torch.isfinite(got).all()), f'{what}: scores are not finite'
    err = (got64.sum(1) - 1).abs().max().item()
    bound = _softmax_ulps(n) * ULP
    assert err <= bound, f'{what}: a softmax row sums to 1 -+ {err:.3g}, allowed {bound:.3g}'
    ref64 = F.softmax(cls.double(), 1)
    top = ref64.topk(2, dim=1).values if n > 1 else None
    if top is not None:
        clear = (top[:, 0] - top[:, 1]) > 2 * bound * top[:, 0]
        assert bool((got.argmax(1).cpu()[clear] == ref64.argmax(1)[clear]).all()), f'{what}: argmax of the scores'
        assert int(clear.sum()) >= min(cls.shape[0], 3) - 1, f'{what}: no row with a clear maximum'
    return ref64


@functools.lru_cache(maxsize=None)
def _worst():
    return {'box': [0.0, 0.0, ''], 'score': [0.0, 0.0, '']}


def _note(kind, err, ref_err, what):
    w = _worst()[kind]
    if err > w[0]:
        w[:] = [err, ref_err, what]


@pytest.mark.parametrize('NC', [1, 2, 62, 63, 64, 126, 127, 128, 129, 300, 1203])
def test_bbox_decode_against_float64(NC):
    from dynamask_amd import ops
    for N in (1, 3, 130):
        for agnostic in (False, True):
            boxes, cls, pred = _decode_inputs(N, NC, agnostic, seed=7 * NC + N + (1000 if agnostic else 0))
            for width in (5, 4):
                rois = _rois_of(boxes, width)
                for max_shape in (CLIP, None):
                    for scale in ((1.0, 1.0), (1.25, 1.6)):
                        what = f'NC {NC} N {N} agnostic {agnostic} rois [N,{width}] max_shape {max_shape} scale {scale}'
                        got_b, got_s = ops.bbox_decode(_dev(rois), _dev(cls), _dev(pred), NC, MEANS, STDS, WH_RATIO_CLIP,
                                                       max_shape=max_shape, scale=scale, class_agnostic=agnostic)
                        b32, s32 = _ref_get_bboxes(boxes, cls, pred, max_shape, scale, MEANS, STDS, torch.float32)
                        b64, s64 = _ref_get_bboxes(boxes, cls, pred, max_shape, scale, MEANS, STDS, torch.float64)
                        assert got_b.shape == b64.shape and got_s.shape == s64.shape
                        e, r, _ = assert_close_via_f64(got_b, b32, b64, what + ': boxes')
                        _note('box', e, r, what)
                        e, r, _ = assert_close_via_f64(got_s, s32, s64, what + ': scores')
                        _note('score', e, r, what)
                        _check_scores(got_s, cls, what)
    w = _worst()
    print(f"\nbbox_decode NC {NC}: largest |product - f64| so far: boxes {w['box'][0]:.3g} (fp32 reference {w['box'][1]:.3g}; "
          f"{w['box'][2]}), scores {w['score'][0]:.3g} (fp32 reference {w['score'][1]:.3g}; {w['score'][2]})")


@pytest.mark.parametrize('NC', [1, 63, 128, 300])
def test_bbox_decode_without_scores_or_deltas(NC):
    """cls_score=None: boxes only.  bbox_pred=None: the RoIs themselves, clipped (with max_shape) and rescaled, once per
    class.  Default means and stds as well."""
    from dynamask_amd import ops
    N = 130
    for agnostic in (False, True):
        boxes, cls, pred = _decode_inputs(N, NC, agnostic, seed=31 * NC + agnostic)
        boxes[5] = torch.tensor([-20.0, -3.0, 500.0, 400.0])                 # clipped on every side
        for width in (5, 4):
            rois = _rois_of(boxes, width)
            for max_shape in (CLIP, None):
                for scale in ((1.0, 1.0), (1.25, 1.6)):
                    what = f'NC {NC} agnostic {agnostic} rois [N,{width}] max_shape {max_shape} scale {scale}'
                    zero, one = (0., 0., 0., 0.), (1., 1., 1., 1.)
                    for means, stds in ((MEANS, STDS), (zero, one)):
                        got_b, got_s = ops.bbox_decode(_dev(rois), None, _dev(pred), NC, means, stds, WH_RATIO_CLIP,
                                                       max_shape=max_shape, scale=scale, class_agnostic=agnostic)
                        assert got_s is None
                        b32, _ = _ref_get_bboxes(boxes, None, pred, max_shape, scale, means, stds, torch.float32)
                        b64, _ = _ref_get_bboxes(boxes, None, pred, max_shape, scale, means, stds, torch.float64)
                        assert_close_via_f64(got_b, b32, b64, what + ': boxes, no scores')
                    got_b, got_s = ops.bbox_decode(_dev(rois), _dev(cls), None, NC, MEANS, STDS, WH_RATIO_CLIP,
                                                   max_shape=max_shape, scale=scale, class_agnostic=agnostic)
                    b32, s32 = _ref_get_bboxes(boxes, cls, None, max_shape, scale, MEANS, STDS, torch.float32)
                    b64, s64 = _ref_get_bboxes(boxes, cls, None, max_shape, scale, MEANS, STDS, torch.float64)
                    nb = 1 if agnostic else NC
                    assert got_b.shape == (N, 4 * nb) and b64.shape == (N, 4)
                    assert_close_via_f64(got_b, b32.repeat(1, nb), b64.repeat(1, nb), what + ': RoIs, no deltas')
                    assert_close_via_f64(got_s, s32, s64, what + ': scores, no deltas')


# ------------------------------------------------------------------------------------------------ cascade_refine
def _first_argmax(v):
    """torch's argmax: the first NaN if there is one, else the first maximum."""
    out = []
    for row in v.numpy():
        nan = np.flatnonzero(np.isnan(row))
        out.append(int(nan[0]) if nan.size else int(np.flatnonzero(row == row.max())[0]))
    return torch.tensor(out, dtype=torch.long)


def _ref_cascade(rois, cls, pred, NC, agnostic, img_tab, dtype):
    label = _first_argmax(cls[:, :NC])
    assert torch.equal(label, cls[:, :NC].argmax(1))
    d = pred if agnostic else torch.gather(pred, 1, torch.stack([label * 4 + k for k in range(4)], 1))
    out = rois.to(dtype).clone()
    for b in range(img_tab.shape[0]):
        rows = rois[:, 0] == b
        if not bool(rows.any()):
            continue
        h, w = img_tab[b].tolist()
        out[rows, 1:] = ref_model.delta2bbox(rois[rows, 1:].to(dtype), d[rows].to(dtype), MEANS, STDS, (h, w), WH_RATIO_CLIP)
    return out, label


@pytest.mark.parametrize('agnostic', [False, True])
@pytest.mark.parametrize('NC', [1, 63, 64, 65, 300])
def test_cascade_refine_against_float64(NC, agnostic):
    from dynamask_amd import ops
    img_tab = torch.tensor([[97.0, 131.0], [60.0, 200.0], [150.0, 45.0]])
    for n in (1, 3, 130):
        boxes, cls, pred = _decode_inputs(n, NC, agnostic, seed=13 * NC + n + (500 if agnostic else 0))
        rois = _rois_of(boxes, 5)
        if n > 4 and NC > 2:
            cls[4] = -2.0
            cls[4, [NC - 1, 1, NC // 2]] = 3.0                 # a tie: the first maximum wins
            cls[5, NC - 1] = float('nan')                      # a NaN counts as the maximum
            cls[6, NC - 2] = float('nan')
            cls[6, NC - 1] = float('nan')                      # the first of two
            cls[7] = torch.randn(NC + 1, generator=torch.Generator().manual_seed(NC)) * 0.1
            cls[7, NC] = 50.0                                  # the background column is the largest and does not count
            cls[8] = 0.5                                       # all equal: class 0
        what = f'NC {NC} n {n} agnostic {agnostic}'
        acc = torch.full_like(cls, 3.0).cuda()
        got = ops.cascade_refine(_dev(rois), _dev(cls), _dev(pred), NC, _dev(img_tab), acc, first=True, class_agnostic=agnostic,
                                 means=MEANS, stds=STDS, wh_ratio_clip=WH_RATIO_CLIP)
        r32, label = _ref_cascade(rois, cls, pred, NC, agnostic, img_tab, torch.float32)
        r64, _ = _ref_cascade(rois, cls, pred, NC, agnostic, img_tab, torch.float64)
        if n > 4 and NC > 2:
            assert label[4:9].tolist() == [1, NC - 1, NC - 2, label[7].item(), 0] and label[7] < NC
        assert torch.equal(got[:, 0].cpu(), rois[:, 0]), what
        assert_close_via_f64(got[:, 1:], r32[:, 1:], r64[:, 1:], what + ': refined RoIs')
        assert np.array_equal(acc.cpu().numpy(), (0 + cls).numpy(), equal_nan=True), what + ': score sum, first stage'
        ops.cascade_refine(None, _dev(cls), None, NC, None, acc, first=False, regress=False)
        assert np.array_equal(acc.cpu().numpy(), (cls + cls).numpy(), equal_nan=True), what + ': score sum, later stage'


# ================================================================================================ 2. NMS
IOU_BAND = 16 * 2.0 ** -24          # about eight fp32 roundings of a value that is at most 1


def _iou64(boxes, off):
    """[M, M] IoU of fp32 boxes in float64, the kernel's formula; 0 / 0 is NaN and compares false."""
    b = boxes.double().numpy()
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1 + off) * (y2 - y1 + off)
    w = np.maximum(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]) + off, 0)
    h = np.maximum(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]) + off, 0)
    inter = w * h
    with np.errstate(invalid='ignore', divide='ignore'):
        return inter / (area[:, None] + area[None] - inter)


def _unpack(mask_words, M):
    """[M, words] int64 from the device -> ([M, M] bool, the bits past column M)."""
    u8 = np.ascontiguousarray(mask_words.cpu().numpy()).view(np.uint8)
    bits = np.unpackbits(u8, axis=1, bitorder='little').astype(bool)
    return bits[:, :M], bits[:, M:]


def _uniform_boxes(M, seed):
    g = torch.Generator().manual_seed(seed)
    ctr = torch.rand(M, 2, generator=g) * 100 + 50
    wh = torch.rand(M, 2, generator=g) * 90 + 5
    return torch.cat([ctr - wh / 2, ctr + wh / 2], 1)          # every coordinate in (2, 198)


def _check_matrix(bits, past, boxes, thr, off, what):
    """The kernel's bits against IoU64 > thr; returns (differing bits, pairs inside the band, pairs)."""
    M = boxes.shape[0]
    iou = _iou64(boxes, off)
    thr32 = float(np.float32(thr))                              # the threshold the kernel was handed
    upper = np.triu(np.ones((M, M), dtype=bool), 1)
    want = (iou > thr32) & upper
    with np.errstate(invalid='ignore'):
        band = (np.abs(iou - thr32) <= IOU_BAND) & upper
    pairs = int(upper.sum())
    assert band.sum() <= 1e-5 * pairs, f'{what}: {int(band.sum())} of {pairs} pairs lie within {IOU_BAND:.3g} of the threshold'
    assert not bits[~upper].any(), f'{what}: bits at or below the diagonal'
    assert not past.any(), f'{what}: bits past column M in the last word'
    diff = (bits != want) & ~band
    assert not diff.any(), f'{what}: {int(diff.sum())} bits differ from IoU64 > {thr}, first at {np.argwhere(diff)[0].tolist()}'
    return int((bits != want).sum()), int(band.sum()), pairs


def _nms_mask(boxes, thr, off):
    from dynamask_amd import ops
    M = boxes.shape[0]
    words = (M + 63) // 64
    sb = _dev(boxes)
    out = Guarded((M, words), torch.int64, 0x5a5a5a5a5a5a5a5a)
    assert _lib().dm_nms_mask(ops._p(sb), M, float(thr), off, ops._p(out.t), ops._stream()) == OK
    out.check(f'dm_nms_mask M {M}')
    return _unpack(out.t, M)


SEG_GAP = 7                          # words between two segments' blocks: no kernel may set a bit there


def _nms_mask_segmented(box_list, thr, off):
    """One launch over the segments of ``box_list`` (an empty one among them), the blocks laid out with gaps."""
    from dynamask_amd import ops
    rows, start, o = [], 0, SEG_GAP
    for b in box_list:
        m = b.shape[0]
        rows.append([start, m, o])
        start += m
        o += m * ((m + 63) // 64) + SEG_GAP
    total = o
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    sb = _dev(torch.cat(box_list))
    out = Guarded((total,), torch.int64, 0x5a5a5a5a5a5a5a5a)
    max_words = max((b.shape[0] + 63) // 64 for b in box_list)
    rc = _lib().dm_nms_mask_segmented(ops._p(sb), len(box_list), ops._p(tab), max_words, float(thr), off, ops._p(out.t), total,
                                      ops._stream())
    assert rc == OK
    out.check('dm_nms_mask_segmented')
    flat = out.t.cpu()
    own = torch.zeros(total, dtype=torch.bool)
    res = []
    for (s, m, o), b in zip(rows, box_list):
        words = (m + 63) // 64
        own[o:o + m * words] = True
        res.append(_unpack(flat[o:o + m * words].view(m, words), m) if m else None)
    assert bool((flat[~own] == 0).all()), 'dm_nms_mask_segmented: a word outside every segment\'s block was written'
    return res


NMS_SIZES = (1, 63, 64, 65, 129, 300)


@pytest.mark.parametrize('thr', [0.5, 0.3])
@pytest.mark.parametrize('off', [0, 1])
def test_nms_matrix_against_float64_iou(off, thr):
    box_list = [_uniform_boxes(M, seed=M + 17 * off) for M in NMS_SIZES]
    tot = [0, 0, 0]
    for boxes in box_list:
        bits, past = _nms_mask(boxes, thr, off)
        r = _check_matrix(bits, past, boxes, thr, off, f'dm_nms_mask M {boxes.shape[0]} offset {off} thr {thr}')
        tot = [a + b for a, b in zip(tot, r)]
    seg = box_list[:3] + [torch.zeros(0, 4)] + box_list[3:]
    for boxes, res in zip(seg, _nms_mask_segmented(seg, thr, off)):
        if res is None:
            continue
        r = _check_matrix(res[0], res[1], boxes, thr, off, f'dm_nms_mask_segmented M {boxes.shape[0]} offset {off} thr {thr}')
        tot = [a + b for a, b in zip(tot, r)]
    print(f'\nNMS matrix offset {off} thr {thr}: {tot[0]} differing bits, {tot[1]} of {tot[2]} pairs inside the band')


PLANTED = torch.tensor([
    [0, 0, 2, 2], [0, 0, 2, 1],              # 0, 1: IoU exactly 0.5 at offset 0 (2 / 4)
    [10, 10, 11, 11], [10, 10, 11, 10],      # 2, 3: IoU exactly 0.5 at offset 1 (2 / 4); at offset 0 box 3 has no area
    [20, 20, 24, 23], [20, 20, 24, 23],      # 4, 5: identical
    [30, 30, 30, 30], [30, 30, 30, 30],      # 6, 7: zero area at one place: 0 / 0 at offset 0, IoU 1 at offset 1
    [45, 45, 42, 42], [40, 40, 46, 46],      # 8, 9: an inverted box inside an ordinary one
    [60, 60, 62, 62], [70, 70, 72, 72],      # 10, 11: disjoint
], dtype=torch.float32)


@pytest.mark.parametrize('off', [0, 1])
def test_nms_matrix_planted_pairs(off):
    """Small-integer coordinates: every IoU is exact in fp32, so no bit may differ from IoU64 > thr (strict)."""
    for thr in (0.5, 0.3):
        iou = _iou64(PLANTED, off)
        want = (iou > float(np.float32(thr))) & np.triu(np.ones((12, 12), dtype=bool), 1)
        assert iou[0 + 2 * off, 1 + 2 * off] == 0.5 and iou[4, 5] == 1.0 and iou[10, 11] == 0.0
        assert np.isnan(iou[6, 7]) if off == 0 else iou[6, 7] == 1.0
        assert bool(want[0 + 2 * off, 1 + 2 * off]) == (thr < 0.5)       # exactly 0.5 does not suppress at 0.5
        assert want[4, 5] and not want[10, 11] and bool(want[6, 7]) == (off == 1)
        bits, past = _nms_mask(PLANTED, thr, off)
        assert np.array_equal(bits, want), f'dm_nms_mask offset {off} thr {thr}: {np.argwhere(bits != want).tolist()}'
        assert not past.any()
        pair_list = [PLANTED[k:k + 2] for k in range(0, 12, 2)] + [PLANTED]
        for k, res in enumerate(_nms_mask_segmented(pair_list, thr, off)):
            idx = slice(2 * k, 2 * k + 2) if k < 6 else slice(0, 12)
            assert np.array_equal(res[0], want[idx, idx]), f'dm_nms_mask_segmented segment {k} offset {off} thr {thr}'
            assert not res[1].any()


# ------------------------------------------------------------------------------------------------ the device greedy pass
REDUCE_SIZES = (1, 63, 0, 64, 65, 128, 129, 1000, 4161)          # 4161 boxes = 66 words: the lane loop's second trip
KEEP_CANARY = -77


@pytest.mark.parametrize('density', [0.0, 0.002, 0.05, 0.9])
def test_nms_reduce_segmented_equals_the_greedy_walk(density):
    from dynamask_amd import ops
    mats = [random_upper_bits(M, density, seed=77 * M + int(density * 1000)) for M in REDUCE_SIZES]
    # box 4160 is the one bit of word 65.  Only box 0 suppresses it, so only the second trip of the lane loop, the one that
    # ORs the kept rows of the first 64 boxes into words 65 and up, removes it.
    mats[-1][:, 4160] = False
    mats[-1][0, 4160] = True
    rows, start, o = [], 0, 0
    for M in REDUCE_SIZES:
        rows.append([start, M, o])
        start += M
        o += M * ((M + 63) // 64)
    flat = np.concatenate([pack_rows(b).reshape(-1) for b in mats if b.shape[0]])
    mask = torch.from_numpy(flat.view(np.int64)).cuda()
    tab = torch.tensor(rows, dtype=torch.int64).cuda()
    B = len(REDUCE_SIZES)
    limits = {-1, 1, 63, 64, 65}
    for b in (mats[4], mats[7], mats[8]):
        limits |= set(max_keeps(b)[-2:])
    for max_keep in sorted(limits):
        keep = Guarded((start,), torch.int32, KEEP_CANARY)
        counts = Guarded((B,), torch.int32, KEEP_CANARY)
        rc = _lib().dm_nms_reduce_segmented(ops._p(mask), B, ops._p(tab), 66, max_keep, ops._p(keep.t), ops._p(counts.t),
                                            ops._stream())
        assert rc == OK
        keep.check('keep')
        counts.check('counts')
        kh, ch = keep.t.cpu().numpy(), counts.t.cpu().numpy()
        for (s, M, _), bits, n in zip(rows, mats, ch.tolist()):
            want = greedy_walk(bits, max_keep)
            what = f'density {density} max_keep {max_keep} segment of {M}'
            assert n == len(want), what
            assert kh[s:s + n].tolist() == want, what
            assert bool((kh[s + n:s + M] == KEEP_CANARY).all()), f'{what}: keep was written past the count'


def test_nms_max_num_zero_means_no_limit():
    """ops.nms and ops.nms_segmented agree at max_num -1, 0 and 1: 0 is "no limit", as in multiclass_nms."""
    from dynamask_amd import ops
    boxes = _uniform_boxes(300, seed=5)
    scores = torch.rand(300, generator=torch.Generator().manual_seed(6))
    order = torch.sort(scores, descending=True, stable=True)[1]
    _, ref_keep = ref_model.nms(boxes, scores, 0.5)
    assert 1 < len(ref_keep) < 300
    for max_num in (-1, 0, 1):
        want = ref_keep.tolist() if max_num <= 0 else ref_keep[:max_num].tolist()
        dets, keep = ops.nms(_dev(boxes), _dev(scores), 0.5, max_num=max_num)
        assert keep.cpu().tolist() == want, max_num
        assert torch.equal(dets.cpu(), torch.cat([boxes[want], scores[want][:, None]], 1))
        k, kept = ops.nms_segmented(_dev(boxes[order]), [300], 0.5, max_num=max_num)
        assert order[k[:int(kept[0])].cpu().long()].tolist() == want, max_num


# ================================================================================================ 3. paste
MASK_SIZES = ((28, 28), (14, 14), (1, 1), (7, 28), (28, 7))
CANVASES = ((1, 1), (1, 300), (300, 1), (33, 17), (211, 307), (1100, 1000))      # the last: a second grid-stride trip
# (kind, threshold): logits through the kernel's sigmoid, fp32 probabilities as they are, raw logits as they are
VARIANTS = (('sigmoid', 0.5), ('sigmoid', 1.0), ('probs', 0.5), ('probs', 1.0), ('raw', 0.0), ('raw', -1.0))


def _paste_boxes(H, W):
    """The box list of a canvas; the big canvas takes two of them."""
    kx = min(2, W - 1) + 0.5                                    # a pixel centre inside the canvas
    ky = min(2, H - 1) + 0.5
    boxes = [
        [0.21 * W + 0.13, 0.17 * H + 0.29, 0.83 * W + 0.41, 0.79 * H + 0.37],      # inside
        [-0.31 * W - 1.3, 0.1 * H, 0.4 * W + 0.7, 0.9 * H + 0.2],                    # over the left border
        [0.2 * W, -0.45 * H - 2.1, 0.9 * W + 0.3, 0.5 * H + 0.6],                    # top
        [0.55 * W, 0.2 * H, 1.4 * W + 3.3, 0.8 * H + 0.9],                           # right
        [0.1 * W, 0.6 * H, 0.7 * W + 0.8, 1.3 * H + 2.7],                            # bottom
        [W + 5.2, H + 5.7, W + 30.1, H + 40.3],                                      # wholly outside
        [-W - 0.4, -H - 0.6, 2 * W + 0.3, 2 * H + 0.9],                              # larger than the canvas
        [0.5 * W + 0.1, 0.1 * H, 0.5 * W + 0.4, 0.9 * H + 1.0],                      # 0.3 px wide
        [kx, 0.1 * H, kx, 0.9 * H + 1.0],                                            # zero width on a pixel centre: 0 / 0
        [0.1 * W, ky + 0.25, 0.9 * W + 1.0, ky + 0.25],                              # zero height
        [kx + 0.25, ky, kx + 0.25, ky],                                              # both
        [0.8 * W + 0.6, 0.2 * H, 0.2 * W - 0.3, 0.8 * H + 0.5],                      # inverted: x1 < x0
        [0.5, 0.5, max(W - 0.5, 1.5), max(H - 0.5, 1.5)],                            # corners on half-integers
        [kx, ky, kx + 5.0, ky + 3.0],                                                # box edge on pixel centres
        [1e8, 1e8, 1e8 + 64, 1e8 + 64],                                              # far away
        [-1e8, -1e8, 1e8, 1e8],                                                      # enormous
    ]
    if H * W > 10 ** 6:
        boxes = [boxes[0], boxes[3]]
    return torch.tensor(boxes, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _paste_inputs(mh, mw, H, W):
    boxes = _paste_boxes(H, W)
    g = torch.Generator().manual_seed(mh * 1000 + mw * 100 + H + 3 * W)
    logits = torch.randn(boxes.shape[0], 1, mh, mw, generator=g) * 3
    return logits, boxes


def _paste64(masks, boxes, H, W):
    """_do_paste_mask over the whole canvas with everything in float64.  Returns (value, NaN coordinate, far outside):
    ``far`` marks the pixels whose sample position s lies outside the mask's support (-1, size) by more than
    1e-5 (1 + |s| + size).  The fp32 position is (g + 1) size / 2 - 1 / 2 with g good to two ulps and three roundings
    after it, within 4 * 2^-24 (|s| + size + 1) of this one: forty times less, so that every precision samples nothing
    there and gives exactly 0."""
    masks, boxes = masks.double(), boxes.double()
    N, _, mh, mw = masks.shape
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    with np.errstate(all='ignore'):
        gy = (torch.arange(H, dtype=torch.float64) + 0.5 - y0) / (y1 - y0) * 2 - 1
        gx = (torch.arange(W, dtype=torch.float64) + 0.5 - x0) / (x1 - x0) * 2 - 1
    gx = torch.where(torch.isinf(gx), torch.zeros_like(gx), gx)
    gy = torch.where(torch.isinf(gy), torch.zeros_like(gy), gy)
    gxx = gx[:, None, :].expand(N, H, W)
    gyy = gy[:, :, None].expand(N, H, W)
    nan = torch.isnan(gxx) | torch.isnan(gyy)
    grid = torch.stack([torch.where(nan, torch.full_like(gxx, -5.0), gxx), torch.where(nan, torch.full_like(gyy, -5.0), gyy)], 3)
    v = F.grid_sample(masks, grid, align_corners=False)[:, 0]
    v[nan] = float('nan')
    sx, sy = ((gxx + 1) * mw - 1) / 2, ((gyy + 1) * mh - 1) / 2

    def outside(s, size):
        m = 1e-5 * (1 + s.abs() + size)
        return (s < -1 - m) | (s > size + m)
    far = (outside(sx, mw) | outside(sy, mh)) & ~nan
    assert bool((v[far] == 0).all())
    return v, nan, far


@functools.lru_cache(maxsize=None)
def _paste_case(mh, mw, H, W, kind):
    """(what the product is handed, apply_sigmoid, v64, NaN pixels, far pixels, max|v32 - v64| of each mask) of a case,
    once."""
    logits, boxes = _paste_inputs(mh, mw, H, W)
    if kind == 'sigmoid':
        given, sig, m32, m64 = logits, True, logits.sigmoid(), logits.double().sigmoid()
    elif kind == 'probs':
        given, sig = logits.sigmoid(), False
        m32, m64 = given, given.double()
    else:
        given, sig, m32, m64 = logits, False, logits, logits.double()
    v64, nan, far = _paste64(m64, boxes, H, W)
    v32 = ref_model.paste_masks(m32, boxes, H, W)[0]
    ref_err = torch.where(nan, torch.zeros_like(v64), (v32.double() - v64).abs()).flatten(1).max(1).values      # per mask
    return given, sig, v64, nan, far, ref_err


@functools.lru_cache(maxsize=None)
def _pasted(mh, mw, H, W, kind, thr):
    """ops.paste_masks of a case, on the host, once: the yardstick of the RLE and multi-image forms."""
    from dynamask_amd import ops
    given, sig = _paste_case(mh, mw, H, W, kind)[:2]
    boxes = _paste_inputs(mh, mw, H, W)[1]
    return ops.paste_masks(_dev(given), _dev(boxes), H, W, threshold=thr, apply_sigmoid=sig).cpu()


def _paste_expectation(v64, nan, far, ref_err, thr, what):
    """(the bits of v64 >= thr, the pixels that may differ, the widest band).  The band of a mask is 4 max|v32 - v64| over
    that mask; a pixel far outside the support is exactly 0 in every precision and may not differ whatever thr is, so it
    does not count as inside the band (at thr = 0 every such pixel sits on the threshold).  The inputs must leave at most
    1e-4 of the pixels inside the band: asserted here, from the float64 values alone."""
    want = v64 >= thr
    want[nan] = 0.0 >= thr                                   # a NaN coordinate samples nothing
    band = 4 * ref_err
    near = ((v64 - thr).abs() <= band[:, None, None]) & ~nan & ~far
    assert float(near.sum()) <= 1e-4 * near.numel(), \
        f'{what}: {int(near.sum())} of {near.numel()} pixels lie within the band (widest {float(band.max()):.3g}) of the threshold'
    return want, near, float(band.max())


@pytest.mark.parametrize('canvas', CANVASES, ids=lambda c: f'{c[0]}x{c[1]}')
@pytest.mark.parametrize('msize', MASK_SIZES, ids=lambda m: f'm{m[0]}x{m[1]}')
def test_paste_masks_against_float64_grid_sample(msize, canvas):
    (mh, mw), (H, W) = msize, canvas
    lines = []
    for kind, thr in VARIANTS:
        given, sig, v64, nan, far, ref_err = _paste_case(mh, mw, H, W, kind)
        what = f'mask {mh}x{mw} canvas {H}x{W} {kind} thr {thr}'
        want, near, band = _paste_expectation(v64, nan, far, ref_err, thr, what)
        share = float(near.sum()) / near.numel()
        got = _pasted(mh, mw, H, W, kind, thr)
        assert got.shape == v64.shape and got.dtype == torch.bool
        diff = got != want
        assert not bool((diff & ~near).any()), \
            f'{what}: {int((diff & ~near).sum())} pixels differ from v64 >= thr outside the band of {band:.3g}'
        if thr > 0:
            assert not bool(got[5].any()) if got.shape[0] > 5 else True, f'{what}: a box wholly outside the canvas'
        lines.append((band, share, int(diff.sum()), what))
    worst = max(lines)
    print(f'\npaste {mh}x{mw} on {H}x{W}: widest band {worst[0]:.3g} ({worst[3]}), largest share inside a band '
          f'{max(l[1] for l in lines):.3g}, differing pixels {sum(l[2] for l in lines)}')


@pytest.mark.parametrize('msize', MASK_SIZES, ids=lambda m: f'm{m[0]}x{m[1]}')
def test_paste_rle_and_multi_forms_give_the_bits_of_paste_masks(msize):
    from dynamask_amd import ops
    mh, mw = msize
    sizes = list(CANVASES[:3]) + [(40, 50)] + list(CANVASES[3:])            # the (40, 50) image has no detection
    for kind, thr in VARIANTS:
        want, masks, boxes, counts = [], [], [], []
        for (H, W) in sizes:
            if (H, W) == (40, 50):
                counts.append(0)
                continue
            given, sig = _paste_case(mh, mw, H, W, kind)[:2]
            b = _paste_inputs(mh, mw, H, W)[1]
            bits = _pasted(mh, mw, H, W, kind, thr)
            rles = ops.paste_rle(_dev(given), _dev(b), H, W, threshold=thr, apply_sigmoid=sig)
            ref = [ref_ops.rle_encode(m.numpy()) for m in bits]
            assert rles == ref, f'paste_rle mask {mh}x{mw} canvas {H}x{W} {kind} thr {thr}'
            want += list(zip(bits, ref))
            masks.append(given)
            boxes.append(b)
            counts.append(b.shape[0])
        masks, boxes = _dev(torch.cat(masks)), _dev(torch.cat(boxes))
        buf, offs, det_sizes = ops.paste_masks_multi(masks, boxes, counts, sizes, threshold=thr, apply_sigmoid=sig)
        buf = buf.cpu()
        assert buf.numel() == sum(h * w for h, w in det_sizes) and len(offs) == len(want)
        for n, ((bits, _), o, (h, w)) in enumerate(zip(want, offs, det_sizes)):
            assert torch.equal(buf[o:o + h * w].view(h, w), bits.to(torch.uint8)), f'paste_masks_multi detection {n} {kind} {thr}'
        rles = ops.paste_rle_multi(masks, boxes, counts, sizes, threshold=thr, apply_sigmoid=sig)
        assert rles == [r for _, r in want], f'paste_rle_multi mask {mh}x{mw} {kind} thr {thr}'


def test_paste_wrappers_refuse_more_masks_than_grid_rows():
    from dynamask_amd import ops
    masks = torch.zeros(65536, 1, 1, 1, device='cuda')
    boxes = torch.zeros(65536, 4, device='cuda')
    with pytest.raises(ValueError, match='at most 65535'):
        ops.paste_masks(masks, boxes, 1, 1)
    with pytest.raises(ValueError, match='at most 65535'):
        ops.paste_rle(masks, boxes, 1, 1)
    with pytest.raises(ValueError, match='at most 65535'):
        ops.rle_encode(torch.zeros(65536, 1, 1, device='cuda', dtype=torch.uint8))
    assert ops.paste_masks(masks[:65535], boxes[:65535], 1, 1).shape == (65535, 1, 1)


# ================================================================================================ 4. RLE
JOINTS = (15, 16, 17, 1023, 1024, 4095, 4096, 4097)


def _patterns(total):
    """Column-major bit vectors [K, total]: the patterns of a size."""
    pats = [np.zeros(total, np.uint8), np.ones(total, np.uint8)]
    first, last = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
    first[0], last[-1] = 1, 1
    pats += [first, last]
    for p in JOINTS:
        if p < total:
            one, run = np.zeros(total, np.uint8), np.zeros(total, np.uint8)
            one[p] = 1
            run[p:p + 40] = 1
            pats += [one, run]
    for period in (16, 32):
        pats.append(((np.arange(total) // (period // 2)) % 2).astype(np.uint8))
        pats.append(1 - pats[-1])
    return np.stack(pats)


def _encode_both_forms(canvas, what):
    """ops.rle_encode of uint8 and bool bitmaps [N, h, w] (host) against the oracle, exactly."""
    from dynamask_amd import ops
    want = [ref_ops.rle_encode(m) for m in canvas]
    t = torch.from_numpy(np.ascontiguousarray(canvas))
    assert ops.rle_encode(t.cuda()) == want, f'{what}: uint8'
    assert ops.rle_encode(t.bool().cuda()) == want, f'{what}: bool'
    assert ops.rle_encode((t * 255).cuda()) == want, f'{what}: uint8 of 255'
    return want


@pytest.mark.parametrize('n', [1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097, 8193])
def test_rle_encode_at_the_unit_joints(n):
    for h, w in ((1, n), (n, 1), (3, -(-n // 3)), (3, n)):
        pats = _patterns(h * w)
        canvas = pats.reshape(-1, w, h).transpose(0, 2, 1)          # column-major vectors -> [K, h, w]
        _encode_both_forms(canvas, f'{h}x{w}')


def test_rle_encode_column_across_two_segments():
    h, w = 5000, 2                                                  # one column spans the 4096-pixel segments 0 and 1
    pats = _patterns(h * w)
    _encode_both_forms(pats.reshape(-1, w, h).transpose(0, 2, 1), f'{h}x{w}')


def test_rle_encode_overflows_the_first_boundary_buffer():
    """A 100 x 100 checkerboard has 9901 boundaries (a run continues across every column joint) and the first buffer
    holds 4096: the re-run of _rle_collect."""
    yy, xx = np.mgrid[0:100, 0:100]
    board = ((yy + xx) % 2).astype(np.uint8)
    want = _encode_both_forms(np.stack([board, 1 - board]), 'checkerboard')
    assert all(len(ref_ops.rle_from_string(w['counts'])) - 1 > 4096 for w in want)


def test_rle_encode_scan_carries_across_chunks():
    """300 masks of 64 x 512 are 2400 (mask, segment) pairs: rle_scan_kernel carries twice.  Rectangles and single pixels;
    the first, the last and a middle mask are empty."""
    rng = np.random.default_rng(300)
    canvas = np.zeros((300, 64, 512), np.uint8)
    for n in range(300):
        if n in (0, 149, 299):
            continue
        for _ in range(3):
            y, x = rng.integers(0, 60), rng.integers(0, 470)
            canvas[n, y:y + rng.integers(1, 40), x:x + rng.integers(1, 40)] = 1
        canvas[n, rng.integers(0, 64, 30), rng.integers(0, 512, 30)] ^= 1
    want = _encode_both_forms(canvas, '300 x 64 x 512')
    assert want[0]['counts'] == want[149]['counts'] == want[299]['counts'] == ref_ops.rle_to_string([64 * 512])
