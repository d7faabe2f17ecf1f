"""FCOS without a device: ``build_detector`` on the reference's ten buildable FCOS configs (tests/golden/
g33_fcos_configs.json), the head's ``state_dict`` keys against the reference head's own, ``load_checkpoint``, the pre-2.0
key rename, what is not built, the lazy exports, the fixture's margins, and the header's launching entry points."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fcos_inputs as fi

BUILDABLE = {
    'r50_caffe': ('ResNet', 50, None), 'r50_caffe_gn': ('ResNet', 50, 32), 'r50_caffe_gn_2x': ('ResNet', 50, 32),
    'r50_caffe_gn_mstrain': ('ResNet', 50, 32), 'r101_caffe_gn': ('ResNet', 101, 32), 'r101_caffe_gn_2x': ('ResNet', 101, 32),
    'r101_caffe_gn_mstrain': ('ResNet', 101, 32), 'x101_64x4d_gn_mstrain': ('ResNeXt', 101, 32), 'center': ('ResNet', 50, 32),
    'center_normbbox_centeronreg_giou': ('ResNet', 50, 32),
}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def cfgs(golden_dir):
    with open(os.path.join(golden_dir, fi.CONFIGS)) as f:
        out = json.load(f)
    with open(os.path.join(golden_dir, fi.DCN_CONFIG)) as f:
        out.update(json.load(f))
    return out


def _build(cfg):
    import dynamask_amd
    torch.manual_seed(0)
    return dynamask_amd.build_detector(cfg['model'], test_cfg=cfg['test_cfg'])


@pytest.fixture(scope='module')
def small():
    """The reduced-width head of the fixture, GN form."""
    from dynamask_amd import dense_heads
    return dense_heads.FCOSHead(test_cfg=dict(fi.TEST_CFGS['gn']), **fi.FORMS['gn'])


# ------------------------------------------------------------------------------------------------ build
@pytest.mark.parametrize('name', sorted(BUILDABLE))
def test_build_fcos_from_the_references_config(cfgs, name):
    import dynamask_amd
    from dynamask_amd import backbones, dense_heads, detectors, necks, registry
    assert set(cfgs) == set(BUILDABLE) | {'dcn'}
    cfg = cfgs[name]
    assert cfg['model']['type'] == 'FCOS'
    before = copy.deepcopy(cfg)
    det = _build(cfg)
    assert cfg == before, 'the build changed the caller\'s config'
    assert type(det) is detectors.FCOS and isinstance(det, detectors.SingleStageDetector)
    assert registry.DETECTORS.get('FCOS') is detectors.FCOS and registry.DETECTORS.get('SingleStageDetector') is detectors.SingleStageDetector
    kind, depth, groups = BUILDABLE[name]
    assert type(det.backbone) is getattr(backbones, kind) and det.backbone.depth == depth
    assert type(det.neck) is necks.FPN and det.with_neck and det.with_bbox
    assert type(det.bbox_head) is dense_heads.FCOSHead and det.bbox_head.num_groups == groups
    assert det.bbox_head.test_cfg == cfg['test_cfg'] and det.bbox_head.train_cfg is None
    assert det.test_cfg == cfg['test_cfg'] and det.pretrained == cfg['model']['pretrained']
    # keys and shapes: the head's are the reference head's own, in its order; the parts' under the reference's prefixes
    got = [(k, list(v.shape)) for k, v in det.state_dict().items()]
    head = [(k[len('bbox_head.'):], s) for k, s in got if k.startswith('bbox_head.')]
    assert head == [(k, s) for k, s in cfg['bbox_head_state_dict']]
    m = registry._to_cfgdict(cfg['model'])
    parts = [('backbone', registry.build_backbone(dict(m.backbone))), ('neck', registry.build_neck(dict(m.neck))),
             ('bbox_head', registry.build_head(dict(m.bbox_head, train_cfg=None, test_cfg=cfg['test_cfg'])))]
    assert got == [(f'{p}.{k}', list(v.shape)) for p, mod in parts for k, v in mod.state_dict().items()]
    assert det.bbox_head.scales[0].scale.dim() == 0
    bias = [k for k, _ in head if k.endswith('.conv.bias')]
    assert bool(bias) == (groups is None or cfg['model']['bbox_head'].get('conv_bias') is True)


@pytest.mark.parametrize('name', ['r50_caffe', 'center_normbbox_centeronreg_giou'])
def test_load_checkpoint_round_trip(cfgs, name, tmp_path):
    from dynamask_amd import detectors
    det = _build(cfgs[name])
    g = torch.Generator().manual_seed(3)
    state = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in det.state_dict().items()}
    meta = {'CLASSES': ('person', 'cat'), 'epoch': 12}
    for prefix in ('', 'module.'):
        path = str(tmp_path / f'ckpt{len(prefix)}.pth')
        torch.save({'state_dict': {prefix + k: v for k, v in state.items()}, 'meta': meta}, path)
        for p in det.parameters():
            p.data.zero_()
        assert detectors.load_checkpoint(det, path, strict=True) == (meta, [], [])
        assert all(torch.equal(v, state[k]) for k, v in det.state_dict().items())


def test_old_predictor_keys_are_renamed(small):
    from dynamask_amd import dense_heads
    g = torch.Generator().manual_seed(5)
    state = {k: torch.randn(v.shape, generator=g) for k, v in small.state_dict().items()}
    old = {k.replace('conv_cls.', 'fcos_cls.').replace('conv_reg.', 'fcos_reg.').replace('conv_centerness.', 'fcos_centerness.'): v
           for k, v in state.items()}
    assert 'fcos_cls.weight' in old and 'conv_cls.weight' not in old
    fresh = dense_heads.FCOSHead(**fi.FORMS['gn'])
    assert fresh.load_state_dict(dict(old), strict=True).missing_keys == []          # (a plain dict: no version metadata)
    assert all(torch.equal(v, state[k]) for k, v in fresh.state_dict().items())
    # inside a detector's state dict, under the head's prefix
    holder = torch.nn.Module()
    holder.bbox_head = dense_heads.FCOSHead(**fi.FORMS['gn'])
    holder.load_state_dict({'bbox_head.' + k: v for k, v in old.items()}, strict=True)
    assert torch.equal(holder.bbox_head.conv_centerness.weight, state['conv_centerness.weight'])
    # a state dict that carries the version keeps its keys: the old names are then unexpected
    versioned = small.state_dict()
    assert versioned._metadata['']['version'] == 1
    renamed = type(versioned)((k.replace('conv_cls.', 'fcos_cls.'), v) for k, v in versioned.items())
    renamed._metadata = versioned._metadata
    with pytest.raises(RuntimeError, match='fcos_cls'):
        fresh.load_state_dict(renamed, strict=True)


# ------------------------------------------------------------------------------------------------ refusals
def test_what_is_not_built_raises_by_name(cfgs, small):
    from dynamask_amd import dense_heads
    kw = fi.FORMS['gn']
    with pytest.raises(NotImplementedError, match='dcn_on_last_conv'):
        dense_heads.FCOSHead(**dict(kw, dcn_on_last_conv=True))
    with pytest.raises(NotImplementedError, match='conv_cfg'):
        dense_heads.FCOSHead(**dict(kw, conv_cfg=dict(type='ConvWS')))
    with pytest.raises(NotImplementedError, match='norm_cfg'):
        dense_heads.FCOSHead(**dict(kw, norm_cfg=dict(type='BN')))
    with pytest.raises(NotImplementedError, match='num_groups=24 does not divide feat_channels=64'):
        dense_heads.FCOSHead(**dict(kw, norm_cfg=dict(type='GN', num_groups=24)))
    for fn in ('forward_train', 'loss', 'get_targets'):
        with pytest.raises(NotImplementedError, match=fn):
            getattr(small, fn)()
    with pytest.raises(NotImplementedError, match='training is not built'):
        small([torch.zeros(1, 64, 2, 2, requires_grad=True)] * 5)
    with pytest.raises(NotImplementedError, match='dcn'):
        _build(cfgs['dcn'])
    det = _build(cfgs['r50_caffe'])
    img, metas = torch.zeros(1, 3, 32, 32), [dict()]
    with pytest.raises(NotImplementedError, match='aug_test'):
        det.aug_test([img, img], [metas, metas])
    with pytest.raises(NotImplementedError, match='aug_test'):
        det.forward_test([img, img], [metas, metas])
    with pytest.raises(NotImplementedError, match='forward_train'):
        det(img, metas, return_loss=True)
    with pytest.raises(NotImplementedError, match='forward_dummy'):
        det.forward_dummy(img)
    with pytest.raises(RuntimeError, match='no CPU fallback'), torch.no_grad():
        det.forward_test([img], [metas])


def test_retinanet_stays_unregistered():
    from dynamask_amd import detectors, registry  # noqa: F401
    assert registry.DETECTORS.get('RetinaNet') is None


def test_registration_and_lazy_exports():
    code = ('import sys\nimport dynamask_amd.dense_heads\nfrom dynamask_amd import registry\n'
            'assert "dynamask_amd.detectors" not in sys.modules\n'
            'assert registry.HEADS.get("FCOSHead") is dynamask_amd.dense_heads.FCOSHead\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))
    code = ('import sys, dynamask_amd\n'
            'assert "dynamask_amd.detectors" not in sys.modules and "dynamask_amd.dense_heads" not in sys.modules\n'
            'h = dynamask_amd.FCOSHead\n'
            'assert "dynamask_amd.dense_heads" in sys.modules and "dynamask_amd.detectors" not in sys.modules\n'
            'd = dynamask_amd.FCOS\n'
            'assert d is dynamask_amd.DETECTORS.get("FCOS") and issubclass(d, dynamask_amd.SingleStageDetector)\n'
            'assert h is sys.modules["dynamask_amd.registry"].HEADS.get("FCOSHead")\n')
    subprocess.check_call([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT))


# ------------------------------------------------------------------------------------------------ the fixture and the header
def test_the_fixture_stands_clear_of_every_edge(golden_dir):
    """The margins the generator computed in float64 from the reference: the ``nms_pre`` cut, the score cut and the NMS
    threshold are each at least 1e-4 away from deciding otherwise, so the GPU tests may demand the reference's set."""
    g = np.load(os.path.join(golden_dir, fi.FIXTURE))
    for form in fi.DETECTION_FORMS:
        m = g[f'{form}_margins']
        assert m.shape == (3,) and float(m.min()) > 1e-4, (form, m)
        for tag in ('plain', 'rescale'):
            for b in range(fi.B):
                d, lab = g[f'{form}_{tag}_dets_{b}'], g[f'{form}_{tag}_labels_{b}']
                assert d.shape == (len(lab), 5) and 0 < len(lab) <= fi.TEST_CFGS[form]['max_per_img']
    # the first two levels are cut by nms_pre and the others are not
    assert [h * w > fi.NMS_PRE for h, w in fi.LEVELS] == [True, True, False, False, False]


def test_the_group_norm_switch_length_is_one_number():
    """``ops.GN_WIDE_MIN_L`` is the library's constant, and every group of the Grid head (at most 12544 floats, by
    contract at most 16384) stays below it."""
    import re
    from dynamask_amd import ops
    with open(os.path.join(ROOT, 'dynamask_amd', 'csrc', 'grid_head.hip')) as f:
        found = re.findall(r'constexpr int GN_WIDE_MIN_L = (\d+);', f.read())
    assert found == [str(ops.GN_WIDE_MIN_L)] and ops.GN_WIDE_MIN_L > 16384


def test_the_header_has_no_new_launching_entry_point():
    import guard_arena
    from dynamask_amd import _lib, hazard
    reached = set().union(*guard_arena.EXPECTED_REACHED.values())
    assert guard_arena.launching(hazard.parse_header()) == reached | set(guard_arena.NO_CALL_SITE)
    assert _lib.ABI_VERSION == 29
