"""FCOS fixture from the REFERENCE's own head: tests/golden/g33_fcos.npz and g33_fcos_configs.json.

    python tests/golden/make_golden_fcos.py REFERENCE_ROOT

Loads ``mmdet/models/dense_heads/{base_dense_head,anchor_free_head,fcos_head}.py`` by path under the stand-ins of
make_golden.py / make_golden_aug.py (``multiclass_nms`` is the reference's own file; ``batched_nms`` delegates to oracle/),
plus stand-ins of its own for the ``mmcv.cnn`` names those files import: a ConvModule with ``bias='auto'`` and GroupNorm
under the key ``gn``, ``Scale``, and initialisers that do nothing (the weights are fcos_inputs.head_state's).  Builds the
reference ``FCOSHead`` in the forms of fcos_inputs.FORMS and runs on the CPU, in float32 and once more in float64:

  * ``forward`` on fcos_inputs.feats(): ``{form}_cls_{l}``, ``{form}_bbox_{l}``, ``{form}_ctr_{l}`` (and ``...64``);
  * for the forms of DETECTION_FORMS, ``get_bboxes`` on those outputs with ``rescale`` False and True:
    ``{form}_{plain|rescale}_dets_{b}`` / ``_labels_{b}`` (and ``_dets64_{b}``).

It also stores the reference's margins per detection form, computed in float64 (``{form}_margins`` = [a, b, c]):
  a  the smallest relative gap between the ``nms_pre``-th key ``max_c(score * centerness)`` and the next, per cut level;
  b  the smallest distance of a candidate row's class score and of its ``score * centerness`` from ``score_thr``;
  c  the smallest distance of a pairwise IoU among same-class candidates from the NMS threshold.
The generator tries the weight seeds of fcos_inputs.WEIGHT_SEEDS until every margin of every form exceeds 1e-4, the float64
run keeps the float32 run's labels, and every image has detections; the seed it settles on is stored as ``weight_seed``.

The JSON holds ``model`` / ``test_cfg`` / ``test_pipeline`` / ``img_norm_cfg`` of the ten buildable files of configs/fcos
as ``registry.Config.fromfile`` resolves them (every ``model`` keeps its ``type``: tools/module_digest.py records no
section for a whole detector), and the reference head's ordered ``state_dict`` keys and shapes.  The ``_dcn_`` file, which
the package refuses, goes to g33_fcos_dcn.json (no ``*_configs.json``: those hold buildable parts), without a key list: its
head needs mmcv's DCNv2."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

CONFIGS = {
    'r50_caffe': 'configs/fcos/fcos_r50_caffe_fpn_4x4_1x_coco.py',
    'r50_caffe_gn': 'configs/fcos/fcos_r50_caffe_fpn_gn-head_4x4_1x_coco.py',
    'r50_caffe_gn_2x': 'configs/fcos/fcos_r50_caffe_fpn_gn-head_4x4_2x_coco.py',
    'r50_caffe_gn_mstrain': 'configs/fcos/fcos_r50_caffe_fpn_gn-head_mstrain_640-800_4x4_2x_coco.py',
    'r101_caffe_gn': 'configs/fcos/fcos_r101_caffe_fpn_gn-head_4x4_1x_coco.py',
    'r101_caffe_gn_2x': 'configs/fcos/fcos_r101_caffe_fpn_gn-head_4x4_2x_coco.py',
    'r101_caffe_gn_mstrain': 'configs/fcos/fcos_r101_caffe_fpn_gn-head_mstrain_640-800_4x4_2x_coco.py',
    'x101_64x4d_gn_mstrain': 'configs/fcos/fcos_x101_64x4d_fpn_gn-head_mstrain_640-800_4x2_2x_coco.py',
    'center': 'configs/fcos/fcos_center_r50_caffe_fpn_gn-head_4x4_1x_coco.py',
    'center_normbbox_centeronreg_giou': 'configs/fcos/fcos_center-normbbox-centeronreg-giou_r50_caffe_fpn_gn-head_4x4_1x_coco.py',
    'dcn': 'configs/fcos/fcos_center-normbbox-centeronreg-giou_r50_caffe_fpn_gn-head_dcn_4x4_1x_coco.py',
}
MARGIN = 1e-4


class TowerConvModule(nn.Module):
    """mmcv ConvModule as the anchor-free heads build it: Conv2d(bias, 'auto' = no norm) -> GroupNorm (key ``gn``) -> ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None, bias='auto',
                 **kw):
        super().__init__()
        assert conv_cfg is None and not kw, (conv_cfg, kw)
        if bias == 'auto':
            bias = norm_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, bias=bias)
        if norm_cfg is not None:
            assert norm_cfg['type'] == 'GN'
            self.gn = nn.GroupNorm(norm_cfg['num_groups'], out_channels)
        self.activate = nn.ReLU(inplace=True)

    def forward(self, x):
        x = self.conv(x)
        if hasattr(self, 'gn'):
            x = self.gn(x)
        return self.activate(x)


class Scale(nn.Module):
    """mmcv.cnn.Scale."""

    def __init__(self, scale=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.tensor(scale, dtype=torch.float))

    def forward(self, x):
        return x * self.scale


def load_fcos_reference(ref):
    import make_golden as mg
    import make_golden_aug as mga
    mg.REF = ref
    R = mga.load_aug_reference()
    cnn = mg._pkg('mmcv.cnn')
    cnn.ConvModule = TowerConvModule
    cnn.Scale = Scale
    cnn.normal_init = lambda m, **k: None
    cnn.bias_init_with_prob = lambda p: 0.0
    core = mg._pkg('mmdet.core')
    core.distance2bbox = sys.modules['mmdet.core.bbox.transforms'].distance2bbox
    mg._pkg('mmdet.models.dense_heads')
    mg._load('mmdet.models.dense_heads.base_dense_head', 'mmdet/models/dense_heads/base_dense_head.py')
    mg._load('mmdet.models.dense_heads.anchor_free_head', 'mmdet/models/dense_heads/anchor_free_head.py')
    R['fcos'] = mg._load('mmdet.models.dense_heads.fcos_head', 'mmdet/models/dense_heads/fcos_head.py')
    return R


def _configs(ref, R):
    from dynamask_amd import registry
    out = {}
    for name, rel in CONFIGS.items():
        cfg = registry.Config.fromfile(os.path.join(ref, rel))
        assert cfg.model['type'] == 'FCOS'
        keys = None
        if name != 'dcn':
            bh = dict(cfg.model.bbox_head)
            bh.pop('type')
            head = R['fcos'].FCOSHead(train_cfg=None, test_cfg=cfg.test_cfg, **bh)
            keys = [[k, list(v.shape)] for k, v in head.state_dict().items()]
        out[name] = {'source': rel, 'model': cfg.model, 'test_cfg': cfg.test_cfg, 'test_pipeline': cfg.test_pipeline,
                     'img_norm_cfg': cfg.img_norm_cfg, 'bbox_head_state_dict': keys}
    return out


def _iou(b):
    """Pairwise IoU [n, n] of boxes [n, 4] (mmcv nms: no +1 offset)."""
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    lt = torch.max(b[:, None, :2], b[None, :, :2])
    rb = torch.min(b[:, None, 2:], b[None, :, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area[:, None] + area[None] - inter)


def margins(head, outs64, metas, cfg):
    """[a, b, c] of the docstring from the float64 head outputs, by the reference's own steps."""
    tr = sys.modules['mmdet.core.bbox.transforms']
    a = b = c = float('inf')
    nms_pre, thr, iou_thr = cfg['nms_pre'], cfg['score_thr'], cfg['nms']['iou_threshold']
    for img in range(len(metas)):
        boxes, scores, ctrs = [], [], []
        for l, (cs, bp, ct) in enumerate(zip(*outs64)):
            H, W = cs.shape[2:]
            s = cs[img].permute(1, 2, 0).reshape(H * W, -1).sigmoid()
            t = ct[img].permute(1, 2, 0).reshape(-1).sigmoid()
            d = bp[img].permute(1, 2, 0).reshape(-1, 4)
            pts = head._get_points_single((H, W), head.strides[l], d.dtype, d.device)
            if H * W > nms_pre:
                key = (s * t[:, None]).max(dim=1)[0]
                ranked, idx = key.sort(descending=True)
                a = min(a, float((ranked[nms_pre - 1] - ranked[nms_pre]) / ranked[nms_pre - 1]))
                idx = idx[:nms_pre]
                s, t, d, pts = s[idx], t[idx], d[idx], pts[idx]
            boxes.append(tr.distance2bbox(pts, d, max_shape=metas[img]['img_shape']))
            scores.append(s)
            ctrs.append(t)
        boxes, scores, ctrs = torch.cat(boxes), torch.cat(scores), torch.cat(ctrs)
        prod = scores * ctrs[:, None]
        b = min(b, float((scores - thr).abs().min()), float((prod - thr).abs().min()))
        valid = scores > thr
        for k in range(scores.shape[1]):
            bx = boxes[valid[:, k]]
            if bx.shape[0] > 1:
                iou = _iou(bx)
                off = ~torch.eye(bx.shape[0], dtype=torch.bool)
                c = min(c, float((iou[off] - iou_thr).abs().min()))
    return [a, b, c]


def run_seed(R, seed, fi):
    """The fixture arrays for one weight seed, or None when a condition of the docstring fails."""
    from dynamask_amd import registry
    out = {'weight_seed': np.array(seed, np.int64)}
    feats = fi.feats()
    for form, kw in fi.FORMS.items():
        cfg = registry._to_cfgdict(fi.TEST_CFGS[form])
        head = R['fcos'].FCOSHead(train_cfg=None, test_cfg=cfg, **kw).eval()
        shapes = {k: tuple(v.shape) for k, v in head.state_dict().items()}
        head.load_state_dict(fi.head_state(shapes, seed, form), strict=True)
        with torch.no_grad():
            outs = head(feats)
            head.double()
            outs64 = head([f.double() for f in feats])
            for nm, o, o64 in zip(('cls', 'bbox', 'ctr'), outs, outs64):
                for l in range(len(o)):
                    out[f'{form}_{nm}_{l}'] = o[l].numpy().astype(np.float32)
                    out[f'{form}_{nm}64_{l}'] = o64[l].numpy()
            if form not in fi.DETECTION_FORMS:
                continue
            m = margins(head, outs64, fi.img_metas(), cfg)
            print(f'  {form}: margins {m}', flush=True)
            if not min(m) > MARGIN:
                return None
            out[f'{form}_margins'] = np.array(m, np.float64)
            for tag, rescale in (('plain', False), ('rescale', True)):
                metas = fi.img_metas(rescaled=rescale)
                r64 = head.get_bboxes(*outs64, metas, rescale=rescale)
                head.float()
                r32 = head.get_bboxes(*outs, metas, rescale=rescale)
                head.double()
                for bi, ((d32, l32), (d64, l64)) in enumerate(zip(r32, r64)):
                    if not torch.equal(l32, l64) or len(l32) == 0:
                        print(f'  {form} {tag} image {bi}: float64 keeps another set, or none', flush=True)
                        return None
                    cand = int((torch.cat([o[bi].permute(1, 2, 0).reshape(-1, fi.NUM_CLASSES) for o in outs[0]]).sigmoid()
                                > cfg['score_thr']).sum())
                    print(f'  {form} {tag} image {bi}: {len(l32)} detections, {cand} scores above the cut before nms_pre', flush=True)
                    out[f'{form}_{tag}_dets_{bi}'] = d32.numpy().astype(np.float32)
                    out[f'{form}_{tag}_labels_{bi}'] = l32.numpy().astype(np.int64)
                    out[f'{form}_{tag}_dets64_{bi}'] = d64.numpy()
    return out


def main(ref):
    import fcos_inputs as fi
    torch.manual_seed(0)
    R = load_fcos_reference(ref)
    out = None
    for seed in fi.WEIGHT_SEEDS:
        print('seed', seed, flush=True)
        out = run_seed(R, seed, fi)
        if out is not None:
            break
    assert out is not None, 'no seed of fcos_inputs.WEIGHT_SEEDS meets the conditions'
    path = os.path.join(HERE, fi.FIXTURE)
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    cfgs = _configs(ref, R)
    # the ``_dcn_`` file apart, under a name that is no ``*_configs.json``: the fixtures of that name hold buildable parts
    for name, part in ((fi.CONFIGS, {k: v for k, v in cfgs.items() if k != 'dcn'}), (fi.DCN_CONFIG, {'dcn': cfgs['dcn']})):
        path = os.path.join(HERE, name)
        with open(path, 'w') as f:
            json.dump(part, f, indent=1, sort_keys=True)
            f.write('\n')
        print('wrote', path, os.path.getsize(path), 'bytes')
        assert os.path.getsize(path) < (1 << 20)


if __name__ == '__main__':
    if len(sys.argv) != 2:
        sys.exit('usage: python tests/golden/make_golden_fcos.py REFERENCE_ROOT')
    main(sys.argv[1])
