"""FCOS on the device: ``FCOSHead.forward`` against the reference head's outputs (tests/golden/g33_fcos.npz, the float64
triangle), ``get_bboxes`` on the reference's own head outputs against the reference's detections (exact membership: the
fixture's margins are asserted in test_fcos_cpu.py), launch and host-wait counts, the detector against its parts composed
by hand, and the wide build of GroupNorm behind ``ops.group_norm`` against ``F.group_norm``."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fcos_inputs as fi
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGES = [(67, 131), (37, 53)]


@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, fi.FIXTURE))


@pytest.fixture(scope='module')
def heads(golden):
    """form -> the head on the device with the fixture's weights."""
    from dynamask_amd import dense_heads
    out = {}
    for form, kw in fi.FORMS.items():
        h = dense_heads.FCOSHead(test_cfg=copy.deepcopy(fi.TEST_CFGS[form]), **kw)
        h.load_state_dict(fi.head_state({k: tuple(v.shape) for k, v in h.state_dict().items()}, int(golden['weight_seed']), form),
                          strict=True)
        out[form] = h.cuda().eval()
    return out


@pytest.fixture(scope='module')
def feats():
    return [f.cuda() for f in fi.feats()]


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the head's forward
@pytest.mark.parametrize('form', sorted(fi.FORMS))
def test_forward_against_the_reference_head(heads, feats, golden, form):
    import dynamask_amd
    h = heads[form]
    with torch.no_grad():
        outs = h(feats)
        for nm, o in zip(('cls', 'bbox', 'ctr'), outs):
            assert len(o) == len(fi.LEVELS)
            for l, t in enumerate(o):
                ref32, ref64 = golden[f'{form}_{nm}_{l}'], golden[f'{form}_{nm}64_{l}']
                assert tuple(t.shape) == ref32.shape
                assert_close_via_f64(t, ref32, ref64, f'{form} {nm} level {l}')
        # image 0 alone has the bits it has in the batch
        alone = h([f[:1].contiguous() for f in feats])
        for a, b in zip(alone, outs):
            for l, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(_bits(x[0]), _bits(y[0])), f'{form} level {l}: an image\'s bits depend on the batch'
        # every convolution is exact fp32 in every precision mode
        with dynamask_amd.conv_precision('bf16x3'):
            again = h(feats)
        for a, b in zip(again, outs):
            for l, (x, y) in enumerate(zip(a, b)):
                assert torch.equal(_bits(x), _bits(y)), f'{form} level {l}: the bf16x3 mode reached the head'


@pytest.mark.parametrize('form', sorted(fi.FORMS))
def test_launches_per_level_and_no_host_wait(heads, feats, form, monkeypatch):
    """The launch table of DESIGN: under GN 13 launches on a level ``ops.conv2d`` takes (layer 0 stacked: 1 convolution +
    1 norm; layers 1 .. 3: 2 + 1; 2 predictors) and 18 on one it does not (4 x (2 + 2) + 2); without a norm 9 and 10.  Of
    the fixture's levels only the 1 x 1 map leaves ``ops.conv2d`` (64 output channels)."""
    import bench
    from dynamask_amd import ops
    h = heads[form]
    with torch.no_grad():
        h(feats)
        assert bench.count_host_syncs(lambda: h(feats)) == 0
    calls = []
    for fn in ('conv2d', 'conv3x3_dil', 'group_norm'):
        def counted(*a, _real=getattr(ops, fn), _fn=fn, **k):
            calls.append(_fn)
            return _real(*a, **k)
        monkeypatch.setattr(ops, fn, counted)
    gn = form != 'nonorm'
    for l, x in enumerate(feats):
        del calls[:]
        with torch.no_grad():
            h.forward_single(x, h.scales[l], h.strides[l])
        if tuple(x.shape[2:]) == (1, 1):
            want = dict(conv2d=0, conv3x3_dil=10, group_norm=8 if gn else 0)
        else:
            want = dict(conv2d=9, conv3x3_dil=0, group_norm=4 if gn else 0)
        assert {fn: calls.count(fn) for fn in want} == want, f'level {l}'
        assert len(calls) == ((18 if gn else 10) if x.shape[2] * x.shape[3] == 1 else (13 if gn else 9))


def test_forward_on_a_wide_map(heads, monkeypatch):
    """A map wider than 168 leaves ops.conv2d for the any-size kernel; it agrees with the same columns run narrow only
    up to rounding, so it is held to torch."""
    from dynamask_amd import ops
    h = heads['gn']
    x = torch.randn(1, fi.CHANNELS, 3, 170, generator=torch.Generator().manual_seed(5))
    monkeypatch.setattr(ops, 'conv2d', lambda *a, **k: pytest.fail('conv2d ran on a 170-wide map'))
    with torch.no_grad():
        cls, box, ctr = h.forward_single(x.cuda(), h.scales[0], h.strides[0])

    def ref(dt):
        p = {k: v.detach().cpu().to(dt) for k, v in h.state_dict().items()}
        c = r = x.to(dt)
        for i in range(4):
            c = F.relu(F.group_norm(F.conv2d(c, p[f'cls_convs.{i}.conv.weight'], None, padding=1), 32, p[f'cls_convs.{i}.gn.weight'], p[f'cls_convs.{i}.gn.bias']))
            r = F.relu(F.group_norm(F.conv2d(r, p[f'reg_convs.{i}.conv.weight'], None, padding=1), 32, p[f'reg_convs.{i}.gn.weight'], p[f'reg_convs.{i}.gn.bias']))
        return (F.conv2d(c, p['conv_cls.weight'], p['conv_cls.bias'], padding=1),
                (F.conv2d(r, p['conv_reg.weight'], p['conv_reg.bias'], padding=1) * p['scales.0.scale']).exp(),
                F.conv2d(c, p['conv_centerness.weight'], p['conv_centerness.bias'], padding=1))
    with torch.no_grad():
        for nm, got, r32, r64 in zip(('cls', 'bbox', 'ctr'), (cls, box, ctr), ref(torch.float32), ref(torch.float64)):
            assert_close_via_f64(got, r32, r64, f'wide map {nm}')


# ------------------------------------------------------------------------------------------------ get_bboxes
def _by_label_and_score(dets, labels):
    dets, labels = np.asarray(dets, np.float64), np.asarray(labels)
    order = np.lexsort((-dets[:, 4], labels))
    return dets[order], labels[order]


@pytest.mark.parametrize('rescale', [False, True])
@pytest.mark.parametrize('form', fi.DETECTION_FORMS)
def test_get_bboxes_on_the_references_head_outputs(heads, golden, form, rescale):
    h = heads[form]
    outs = [[torch.from_numpy(golden[f'{form}_{nm}_{l}']).cuda() for l in range(len(fi.LEVELS))] for nm in ('cls', 'bbox', 'ctr')]
    tag = 'rescale' if rescale else 'plain'
    with torch.no_grad():
        got = h.get_bboxes(*outs, fi.img_metas(rescaled=rescale), rescale=rescale)
    assert len(got) == fi.B
    for b, (dets, labels) in enumerate(got):
        ref_d, ref_l = golden[f'{form}_{tag}_dets_{b}'], golden[f'{form}_{tag}_labels_{b}']
        assert dets.dtype == torch.float32 and labels.dtype == torch.int64 and dets.shape == (labels.shape[0], 5)
        assert labels.shape[0] == ref_l.shape[0], f'image {b}: {labels.shape[0]} detections, the reference keeps {ref_l.shape[0]}'
        # in the reference's order: descending score
        s = dets[:, 4].cpu().numpy()
        assert (s[:-1] >= s[1:]).all()
        gd, gl = _by_label_and_score(dets.cpu().numpy(), labels.cpu().numpy())
        rd, rl = _by_label_and_score(ref_d, ref_l)
        assert np.array_equal(gl, rl), f'image {b}: other labels'
        err = np.abs(gd - rd) / np.maximum(1.0, np.abs(rd))
        print(f'{form} {tag} image {b}: {len(rl)} detections, worst |got - ref| / max(1, |ref|) = {err.max():.3g}')
        assert err.max() <= 1e-5, f'image {b}: {err.max():.3g}'


def test_an_empty_image_and_the_one_host_wait(heads, golden):
    import bench
    h = heads['gn']
    outs = [[torch.from_numpy(golden[f'gn_{nm}_{l}']).cuda() for l in range(len(fi.LEVELS))] for nm in ('cls', 'bbox', 'ctr')]
    metas = fi.img_metas()
    with torch.no_grad():
        h.get_bboxes(*outs, metas, rescale=True)
        assert bench.count_host_syncs(lambda: h.get_bboxes(*outs, metas, rescale=True)) == 1
        # image 1 with every score under score_thr (sigmoid(-20) = 2e-9); image 0 keeps its detections
        outs[0] = [torch.cat([c[:1], torch.full_like(c[1:], -20.0)]) for c in outs[0]]
        got = h.get_bboxes(*outs, metas, rescale=False)
    assert tuple(got[1][0].shape) == (0, 5) and tuple(got[1][1].shape) == (0,) and got[1][1].dtype == torch.int64
    assert got[0][1].shape[0] == golden['gn_plain_labels_0'].shape[0]
    with torch.no_grad():
        one = h.get_bboxes(*[[t[1:] for t in o] for o in outs], metas[1:])
    assert len(one) == 1 and tuple(one[0][0].shape) == (0, 5) and tuple(one[0][1].shape) == (0,)


def test_a_cap_below_the_candidate_count_gives_the_same_detections(heads, golden, monkeypatch):
    """More candidates than NMS_CANDIDATE_CAP: the call runs again, wider, and returns what the uncapped call returns."""
    from dynamask_amd import dense_heads
    h = heads['tricks']
    outs = [[torch.from_numpy(golden[f'tricks_{nm}_{l}']).cuda() for l in range(len(fi.LEVELS))] for nm in ('cls', 'bbox', 'ctr')]
    with torch.no_grad():
        want = h.get_bboxes(*outs, fi.img_metas(), rescale=True)
        monkeypatch.setattr(dense_heads, 'NMS_CANDIDATE_CAP', 64)
        got = h.get_bboxes(*outs, fi.img_metas(), rescale=True)
    for (d, l), (wd, wl) in zip(got, want):
        assert torch.equal(_bits(d), _bits(wd)) and torch.equal(l, wl)


# ------------------------------------------------------------------------------------------------ the detector
@pytest.fixture(scope='module')
def detector(golden_dir, golden):
    """(FCOS at reduced head and neck width on the device, its parts built one by one with the same weights, cfg)."""
    import backbone_inputs as bi
    import fpn_inputs as fpi
    from dynamask_amd import build_detector, registry
    with open(os.path.join(golden_dir, fi.CONFIGS)) as f:
        cfg = json.load(f)['r50_caffe_gn']
    cfg['model']['neck']['out_channels'] = fi.CHANNELS
    cfg['model']['bbox_head'].update(num_classes=fi.NUM_CLASSES, in_channels=fi.CHANNELS, feat_channels=fi.CHANNELS)
    cfg['test_cfg'].update(nms_pre=fi.NMS_PRE, max_per_img=20)
    cfg['test_pipeline'][1]['img_scale'] = [160, 96]
    det = build_detector(copy.deepcopy(cfg['model']), test_cfg=copy.deepcopy(cfg['test_cfg']))
    own = det.state_dict()
    state = {}
    for part, fn in (('backbone', bi.head_state), ('neck', fpi.head_state),
                     ('bbox_head', lambda s, seed: fi.head_state(s, seed, 'gn'))):
        shapes = {k[len(part) + 1:]: tuple(v.shape) for k, v in own.items() if k.startswith(part + '.')}
        state.update({f'{part}.{k}': v for k, v in fn(shapes, int(golden['weight_seed'])).items()})
    det.load_state_dict(state, strict=True)
    m = registry._to_cfgdict(cfg['model'])
    parts = {'backbone': registry.build_backbone(dict(m.backbone)), 'neck': registry.build_neck(dict(m.neck)),
             'bbox_head': registry.build_head(dict(m.bbox_head, train_cfg=None, test_cfg=registry._to_cfgdict(cfg['test_cfg'])))}
    for part, mod in parts.items():
        mod.load_state_dict({k[len(part) + 1:]: v for k, v in state.items() if k.startswith(part + '.')}, strict=True)
        parts[part] = mod.cuda().eval()
    return det.cuda().eval(), parts, cfg


def _images(n=2):
    rng = np.random.default_rng(33)
    return [torch.from_numpy(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).cuda() for h, w in IMAGES[:n]]


def _same(a, b):
    assert type(a) is type(b)
    if isinstance(a, list):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    else:
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('n', [1, 2])
def test_simple_test_is_the_parts_composed(detector, n):
    from dynamask_amd import detectors, postprocess
    det, parts, cfg = detector
    img, metas = detectors.preprocess(_images(n), cfg['img_norm_cfg'], size_divisor=32)
    assert tuple(img.shape) == (n, 3, 96, 160)
    with torch.no_grad():
        for rescale in (False, True):
            got = det.simple_test(img, metas, rescale=rescale)
            outs = parts['bbox_head'](parts['neck'](parts['backbone'](img)))
            bbox_list = parts['bbox_head'].get_bboxes(*outs, metas, rescale=rescale)
            want = [postprocess.bbox2result(d, l, fi.NUM_CLASSES) for d, l in bbox_list]
            _same(got, want[0] if n == 1 else want)
            assert sum(len(r) for res in want for r in res) > 0, 'no detection: the comparison would check nothing'
        _same(det.forward_test([img], [metas], rescale=True), got)
        _same(det(img=[img], img_metas=[metas], rescale=True), got)


def test_detect_and_aug_test(detector):
    from dynamask_amd import detectors
    det, _, cfg = detector
    images = _images(2)
    p = detectors.parse_test_pipeline(cfg)
    with torch.no_grad():
        got = det.detect(images, cfg)
        img, metas = detectors.preprocess(images, p['img_norm_cfg'], img_scale=p['img_scales'][0], keep_ratio=True,
                                          size_divisor=p['size_divisor'])
        _same(got, det.simple_test(img, metas, rescale=True))
        _same(det.detect([im.cpu().numpy() for im in images[:1]], cfg), det.detect(images[:1], cfg))
        with pytest.raises(NotImplementedError, match='aug_test'):
            det.aug_test([img, img], [metas, metas])
        flipped = copy.deepcopy(cfg['test_pipeline'])
        flipped[1]['flip'] = True
        with pytest.raises(NotImplementedError, match='aug_test'):
            det.detect(images[:1], flipped)


# ------------------------------------------------------------------------------------------------ GroupNorm, the wide build
def _gn_case(shape, G, seed=0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 2.0 + mean
    C = shape[1]
    return x, 1.0 + 0.2 * torch.randn(C, generator=g), 0.3 * torch.randn(C, generator=g)


def _gn_ref(x, gamma, beta, G, relu, dt):
    y = F.group_norm(x.to(dt), G, gamma.to(dt), beta.to(dt), eps=1e-5)
    return F.relu(y) if relu else y


def _gn_check(ops, shape, G, relu, inplace, name, mean=0.0):
    x, gamma, beta = _gn_case(shape, G, mean=mean)
    xd = x.cuda()
    keep = xd.clone()
    got = ops.group_norm(xd, gamma.cuda(), beta.cuda(), G, relu=relu, out=xd if inplace else None)
    if inplace:
        assert got.data_ptr() == xd.data_ptr()
    else:
        assert torch.equal(xd, keep), f'{name}: the input was written'
    assert_close_via_f64(got, _gn_ref(x, gamma, beta, G, relu, torch.float32), _gn_ref(x, gamma, beta, G, relu, torch.float64), name)
    again = ops.group_norm(keep, gamma.cuda(), beta.cuda(), G, relu=relu)
    assert torch.equal(_bits(again), _bits(got)), f'{name}: two runs, other bits'


WIDE_SHAPES = [((1, 16, 100, 168), 2),          # the stride-8 group of a 1333 x 800 image: 8 x 100 x 168 floats
               ((2, 2, 181, 183), 2)]           # L = 33123, odd: group 1 and sample 1 start off a 16-byte boundary, ragged tail


@pytest.mark.parametrize('inplace', [False, True])
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('shape,G', WIDE_SHAPES)
def test_group_norm_wide(shape, G, relu, inplace):
    from dynamask_amd import ops
    assert (shape[1] // G) * shape[2] * shape[3] >= ops.GN_WIDE_MIN_L
    _gn_check(ops, shape, G, relu, inplace, f'group_norm {shape} G={G} relu={relu} inplace={inplace}')


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_group_norm_on_both_sides_of_the_switch(delta):
    from dynamask_amd import ops
    L = ops.GN_WIDE_MIN_L + delta
    for relu, inplace in ((False, False), (True, True)):
        _gn_check(ops, (1, 1, 1, L), 1, relu, inplace, f'group_norm L = L* {delta:+d} relu={relu}')
    # a group that starts 4, 8 and 12 bytes past a 16-byte boundary: x and y are views into wider buffers
    x, gamma, beta = _gn_case((1, 1, 1, L), 1, seed=3)
    r32, r64 = (_gn_ref(x, gamma, beta, 1, False, dt) for dt in (torch.float32, torch.float64))
    for off_x in (1, 2, 3):
        for off_y in (0, off_x):
            bx, by = torch.zeros(L + 8).cuda(), torch.full((L + 8,), 7.0).cuda()
            xv, yv = bx[off_x:off_x + L].view(1, 1, 1, L), by[off_y:off_y + L].view(1, 1, 1, L)
            xv.copy_(x)
            ops.group_norm(xv, gamma.cuda(), beta.cuda(), 1, out=yv)
            assert_close_via_f64(yv, r32, r64, f'group_norm L = L* {delta:+d}, x + {off_x}, y + {off_y}')
            assert bool((by[:off_y] == 7.0).all()) and bool((by[off_y + L:] == 7.0).all()), 'a store outside the group'


def test_group_norm_wide_contract():
    """A constant group gives exactly beta; a group with mean 1e3 passes; one NaN poisons exactly its group and the other
    groups keep the clean run's bits."""
    from dynamask_amd import ops
    shape, G = (2, 4, 90, 97), 2                    # L = 17460, odd rows
    x, gamma, beta = _gn_case(shape, G, seed=1)
    assert 2 * 90 * 97 >= ops.GN_WIDE_MIN_L
    x[1, 2:4] = 3.25                                # sample 1, group 1: constant
    got = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), G).cpu()
    assert torch.equal(got[1, 2:4], beta[2:4, None, None].expand(2, 90, 97))
    _gn_check(ops, shape, G, True, False, 'group_norm mean 1e3', mean=1e3)
    clean = ops.group_norm(x.cuda(), gamma.cuda(), beta.cuda(), G, relu=True).cpu()
    bad = x.clone()
    bad[0, 1, 45, 50] = float('nan')                # sample 0, group 0
    got = ops.group_norm(bad.cuda(), gamma.cuda(), beta.cuda(), G, relu=True).cpu()
    assert bool(torch.isnan(got[0, 0:2]).all())
    rest = torch.ones(shape, dtype=torch.bool)
    rest[0, 0:2] = False
    assert torch.equal(_bits(got[rest]), _bits(clean[rest])) and not bool(torch.isnan(got[rest]).any())


def test_dm_gn_wide_0_keeps_the_old_build_in_a_fresh_process():
    """DM_GN_WIDE=0 is read when the library first launches: a child process with it set runs a group above L* on the
    narrow build and passes the same comparison."""
    code = (
        'import sys, torch\n'
        'import torch.nn.functional as F\n'
        f'sys.path.insert(0, {os.path.join(ROOT, "tests")!r})\n'
        'from tolerances import assert_close_via_f64\n'
        'from dynamask_amd import ops\n'
        'g = torch.Generator().manual_seed(0)\n'
        'x = torch.randn(2, 2, 181, 183, generator=g) * 2\n'
        'w, b = 1 + 0.2 * torch.randn(2, generator=g), 0.3 * torch.randn(2, generator=g)\n'
        'assert 181 * 183 >= ops.GN_WIDE_MIN_L\n'
        'got = ops.group_norm(x.cuda(), w.cuda(), b.cuda(), 2, relu=True)\n'
        'ref = [F.relu(F.group_norm(x.to(dt), 2, w.to(dt), b.to(dt), eps=1e-5)) for dt in (torch.float32, torch.float64)]\n'
        'assert_close_via_f64(got, ref[0], ref[1], "group_norm under DM_GN_WIDE=0")\n'
        'print("narrow build ok")\n')
    out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT, DM_GN_WIDE='0'),
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and 'narrow build ok' in out.stdout, out.stdout + out.stderr
