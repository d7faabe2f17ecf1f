"""ResNeXt inference on the device: the grouped 3x3 kernel (dm_conv3x3_grouped_fwd) against torch's CPU convolution in
float32 and float64, its batch independence, group isolation with NaN and Inf, its argument checks; ``backbones.ResNeXt``
against the reference's own module (tests/golden/g30_resnext.npz) and, stage by stage, against resnext_inputs.restate; the
launch count, host waits, and the chain through the detector."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ the kernel
# (channels per group, groups): layer1 and layer2 of 32x4d at full group count; the others at the fewest groups that
# cross a group boundary; three groups (no power of two) and one group.
GROUPINGS = [(4, 32), (8, 32), (16, 2), (32, 2), (64, 1), (4, 3), (4, 1)]
# The kernel's output tile (csrc/conv_grouped.hip) is 32 columns wide and 32 / 16 / 8 rows high at 4 / 8 / >= 16 channels
# per group, at both strides; a lane stores 4 neighbouring columns, as one float4 where Wo % 4 == 0.  Of the issue's maps
#   (3, 37, 53) at stride 1 crosses every row edge (37 > 32) and the column edge (53 = 32 + 21); at stride 2 (19 x 27) the
#               row edges of the 16- and 8-row tiles;
#   (1, 5, 130) has 5 tile columns at stride 1 (the last of 2 columns, scalar stores) and 3 at stride 2 (65 = 2 * 32 + 1);
# and the added
#   (1, 67, 40) crosses the 32-row edge at stride 2 too (34 rows = 32 + 2; 67 = 2 * 32 + 3 at stride 1) and takes the
#               float4 stores at both strides (Wo = 40 = 32 + 8 and Wo = 20), which no map of the issue's list does.
MAPS = [(1, 1, 1), (1, 2, 3), (1, 7, 9), (2, 10, 14), (3, 37, 53), (1, 5, 130), (1, 67, 40)]


def _problem(NB, cg, groups, H, W, seed):
    C = cg * groups
    x = torch.randn(NB, C, H, W, generator=_g(seed))
    w = torch.randn(C, cg, 3, 3, generator=_g(seed + 1)) * (2.0 / (9 * cg)) ** 0.5
    b = torch.randn(C, generator=_g(seed + 2)) * 0.5
    return x, w, b


@pytest.mark.parametrize('cg,groups', GROUPINGS, ids=lambda v: str(v))
def test_conv3x3_grouped_against_torch(cg, groups):
    from dynamask_amd import ops
    C = cg * groups
    for NB, H, W in MAPS:
        x, w, b = _problem(NB, cg, groups, H, W, 3000 + 100 * H + W + cg + groups)
        xd, bd = x.cuda(), b.cuda()
        wq = ops.pack_grouped_conv_weight(w.cuda(), groups)
        for stride in (1, 2):
            assert ops.conv3x3_grouped_supported(x, groups, stride)
            for relu in (False, True):
                for bias in (True, False):
                    ref32 = F.conv2d(x, w, b if bias else None, stride, 1, groups=groups)
                    ref64 = F.conv2d(x.double(), w.double(), b.double() if bias else None, stride, 1, groups=groups)
                    if relu:
                        ref32, ref64 = F.relu(ref32), F.relu(ref64)
                    got = ops.conv3x3_grouped(xd, wq, bd if bias else None, groups, stride=stride, relu=relu)
                    name = f'conv3x3_grouped cg={cg} groups={groups} {(NB, H, W)} stride={stride} relu={relu} bias={bias}'
                    assert tuple(got.shape) == (NB, C, (H + stride - 1) // stride, (W + stride - 1) // stride) == tuple(ref32.shape), name
                    assert got.is_contiguous(), name
                    err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, name)
                    print(f'{name}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
                    out = torch.full_like(got, float('nan'))
                    assert ops.conv3x3_grouped(xd, wq, bd if bias else None, groups, stride=stride, relu=relu, out=out) is out
                    assert torch.equal(_bits(out), _bits(got)), name + ': a second call, into a given out, gives other bits'
        assert torch.equal(xd.cpu(), x), 'x was written'


@pytest.mark.parametrize('cg,groups', [(4, 32), (8, 3), (16, 2), (32, 2), (64, 1)], ids=lambda v: str(v))
def test_image_bits_do_not_depend_on_the_batch(cg, groups):
    from dynamask_amd import ops
    x, w, b = _problem(3, cg, groups, 37, 53, 3100 + cg)
    xd, bd, wq = x.cuda(), b.cuda(), ops.pack_grouped_conv_weight(w.cuda(), groups)
    for stride in (1, 2):
        batch = ops.conv3x3_grouped(xd, wq, bd, groups, stride=stride, relu=True)
        for i in range(3):
            alone = ops.conv3x3_grouped(xd[i:i + 1].contiguous(), wq, bd, groups, stride=stride, relu=True)
            assert torch.equal(_bits(alone[0]), _bits(batch[i])), f'stride {stride}, image {i}'


@pytest.mark.parametrize('cg,groups', [(4, 8), (32, 2)], ids=lambda v: str(v))
def test_a_nan_or_an_inf_stays_in_its_group(cg, groups):
    """One NaN, then one +Inf, at one pixel of one input channel: the output channels of every other group keep the clean
    run's bits (no product with another group's input is formed, not even by zero), the poisoned group's have torch's
    pattern."""
    from nonfinite_cases import assert_same_nonfinite
    from dynamask_amd import ops
    C, H, W = cg * groups, 7, 9
    x, w, b = _problem(1, cg, groups, H, W, 3200 + cg)
    bad_group = groups - 1 if groups == 2 else 5
    ch = bad_group * cg + cg // 2
    wq, bd = ops.pack_grouped_conv_weight(w.cuda(), groups), b.cuda()
    others = [c for c in range(C) if c // cg != bad_group]
    own = [c for c in range(C) if c // cg == bad_group]
    for stride in (1, 2):
        clean = ops.conv3x3_grouped(x.cuda(), wq, bd, groups, stride=stride, relu=True).cpu()
        assert bool(torch.isfinite(clean).all())
        for special in (float('nan'), float('inf')):
            xs = x.clone()
            xs[0, ch, 2, 4] = special                # (an even row and column: a centre tap at stride 2)
            got = ops.conv3x3_grouped(xs.cuda(), wq, bd, groups, stride=stride, relu=True).cpu()
            name = f'cg={cg} stride={stride} special={special}'
            assert torch.equal(_bits(got[:, others]), _bits(clean[:, others])), name + ': another group changed'
            ref32 = F.relu(F.conv2d(xs, w, b, stride, 1, groups=groups))
            ref64 = F.relu(F.conv2d(xs.double(), w.double(), b.double(), stride, 1, groups=groups))
            assert torch.equal(torch.isnan(got), torch.isnan(ref32)), name + ': isnan pattern'
            assert bool(torch.isfinite(ref32[:, others]).all()), name
            if special != special:       # every window over the pixel, in every output channel of the group
                assert int(torch.isnan(got[:, own]).sum()) == int(torch.isnan(got).sum()) == cg * (9 if stride == 1 else 1), name
            else:                        # +-Inf by the sign of the weight; the ReLU turns -Inf into 0
                assert_same_nonfinite(got, ref32, ref64, name)


def test_argument_checks():
    from dynamask_amd import _lib, ops
    L = _lib.lib()
    x, w, b = _problem(1, 8, 4, 9, 11, 3300)
    xd, wq = x.cuda(), ops.pack_grouped_conv_weight(w.cuda(), 4)
    out = torch.empty(1, 32, 9, 11).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(xp=p(xd), wp=p(wq), op=p(out), C=32, groups=4, stride=1, flags=0, NB=1):
        return L.dm_conv3x3_grouped_fwd(xp, NB, C, 9, 11, wp, None, groups, stride, flags, op, None)
    assert call() == 0
    assert call(flags=1) == 0 and call(flags=8) == 0 and call(flags=9) == 0
    assert call(flags=16) == -3 and call(flags=17) == -3                  # bf16x3: unsupported
    assert call(flags=2) == -1 and call(flags=4) == -1 and call(flags=32) == -1 and call(flags=1 << 20) == -1
    assert call(xp=None) == -1 and call(wp=None) == -1 and call(op=None) == -1
    for groups in (16, 32, 3, 0):                   # 2 and 1 channels per group; C no multiple of groups; no group
        assert L.dm_conv3x3_grouped_supported(1, 32, 9, 11, groups, 1) == 0 and call(groups=groups) == -3
    for C in (48, 12, 512):                         # 12, 3 and 128 channels per group
        assert L.dm_conv3x3_grouped_supported(1, C, 9, 11, 4, 1) == 0 and call(C=C) == -3
    assert L.dm_conv3x3_grouped_supported(1, 32, 9, 11, 4, 3) == 0 and call(stride=3) == -3 and call(stride=0) == -3
    assert call(NB=0, xp=None, wp=None, op=None) == 0                      # nothing to do
    assert call(NB=-1) == -3
    # the wrapper
    marked = wq.clone()
    marked._dm_bf16x3 = True               # what pack_conv_weight(precision='bf16x3') marks its result with
    with pytest.raises(RuntimeError, match='dm_conv3x3_grouped_fwd'):
        ops.conv3x3_grouped(xd, marked, None, 4)
    with pytest.raises(AssertionError):
        ops.conv3x3_grouped(xd, wq, None, 2)
    with pytest.raises(NotImplementedError, match='stride=3'):
        ops.conv3x3_grouped(xd, wq, None, 4, stride=3)
    with pytest.raises(RuntimeError, match='MI355X only'):
        ops.conv3x3_grouped(x, wq, None, 4)
    assert ops.conv3x3_grouped(torch.zeros(0, 32, 9, 11).cuda(), wq, None, 4, stride=2).shape == (0, 32, 5, 6)
    assert not ops.conv3x3_grouped_supported((1, 32, 9, 11), 16, 1) and ops.conv3x3_grouped_supported((1, 32, 9, 11), 4, 2)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the module
CAFFE = dict(depth=50, groups=64, base_width=4, style='caffe', num_stages=3, strides=(1, 2, 2), dilations=(1, 1, 1),
             out_indices=(2,), frozen_stages=-1)


@pytest.fixture(scope='module')
def nets(golden_dir):
    """({form: ResNeXt on the device with seeded weights}, {form: the seeded state}, {form: the backbone config},
    resnext_inputs, the fixture's images on the device): the fixture's x101-32x4d and the caffe-style 64-group net."""
    import resnext_inputs as xi
    from dynamask_amd import backbones, registry
    with open(os.path.join(golden_dir, xi.CONFIGS)) as f:
        cfgs = json.load(f)
    cfg = {'x101_32x4d': cfgs['x101_32x4d']['model']['backbone'], 'caffe_64x4d': dict(CAFFE, type='ResNeXt')}
    mods, states = {}, {}
    for form in cfg:
        m = registry.build_backbone(copy.deepcopy(cfg[form]))
        assert type(m) is backbones.ResNeXt
        states[form] = xi.head_state({k: v.shape for k, v in m.state_dict().items()}, xi.WEIGHT_SEED)
        assert list(states[form]) == sorted(xi.state_shapes(cfg[form]))
        m.load_state_dict(states[form], strict=True)
        mods[form] = m.cuda().eval()
    return mods, states, cfg, xi, xi.inputs().cuda()


@pytest.fixture(scope='module')
def stage_refs(nets):
    """{form: (stem, [stage outputs])} of resnext_inputs.restate in float32 on the CPU, computed once."""
    _, states, cfg, xi, _ = nets
    with torch.no_grad():
        return {form: xi.restate(cfg[form], states[form], xi.inputs(), every_stage=True) for form in cfg}


def test_forward_against_the_reference(nets, golden_dir):
    from dynamask_amd import conv_precision
    mods, _, cfg, xi, img = nets
    z = np.load(os.path.join(golden_dir, xi.FILE))
    m = mods['x101_32x4d']
    before = img.clone()
    with torch.no_grad():
        outs = m(img)
        again = m(img)
        with conv_precision('bf16x3'):
            outs3 = m(img)
    assert torch.equal(_bits(img), _bits(before)), 'forward wrote into its input'
    assert isinstance(outs, tuple) and len(outs) == 4
    for l, (got, second, other) in enumerate(zip(outs, again, outs3)):
        ref32 = z[f'x101_32x4d_out{l}']
        assert tuple(got.shape) == ref32.shape, f'output {l}'
        err, ref_err, scale = assert_close_via_f64(got, ref32, xi.unpack_f64(ref32, z[f'x101_32x4d_out{l}_err16']), f'output {l}')
        print(f'x101_32x4d output {l}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
        assert torch.equal(_bits(got), _bits(second)), f'output {l}: a second call gives other bits'
        assert torch.equal(_bits(got), _bits(other)), f'output {l}: the bf16x3 mode changed the backbone'


@pytest.mark.parametrize('form', ['x101_32x4d', 'caffe_64x4d'])
def test_every_stage_on_the_references_input(nets, stage_refs, form):
    """Every stage on the float32 restatement's own input to it: an error shows at the stage that makes it.  The caffe
    form strides in conv1 (``ops.subsample2`` in front of the block) and has 64 groups of 4, 8 and 16 channels."""
    mods, states, cfg, xi, img = nets
    m = mods[form]
    stem32, stages32 = stage_refs[form]
    with torch.no_grad():
        x = stem32
        for i, ref32 in enumerate(stages32):
            ref64 = xi.restate_stage(cfg[form], states[form], i, x.double())
            xd = x.cuda()
            keep = xd.clone()
            got = m.run_stage(i, xd)
            assert torch.equal(_bits(xd), _bits(keep)), f'{form} stage {i} wrote into its input'
            err, ref_err, scale = assert_close_via_f64(got, ref32, ref64, f'{form} stage {i}')
            print(f'{form} stage {i}: err {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale:.3g}')
            x = ref32


def test_launches_host_waits_and_batch_independence(nets, monkeypatch):
    import bench
    from dynamask_amd import ops
    mods, _, _, _, img = nets
    m = mods['x101_32x4d']
    with torch.no_grad():
        both = m(img)
        alone = m(img[:1].contiguous())
        assert bench.count_host_syncs(lambda: m(img)) == 0
    for l, (a, b) in enumerate(zip(alone, both)):
        assert torch.equal(_bits(a[0]), _bits(b[0])), f'output {l}: an image\'s bits depend on the batch'
    grouped = []
    real = ops.conv3x3_grouped
    monkeypatch.setattr(ops, 'conv3x3_grouped', lambda x, w, b, groups, **k: (grouped.append((tuple(x.shape), groups, k.get('stride', 1))),
                                                                              real(x, w, b, groups, **k))[1])
    monkeypatch.setattr(ops, 'conv3x3_s2', lambda *a, **k: pytest.fail('a dense stride-2 3x3 ran'))
    monkeypatch.setattr(ops, 'conv3x3_dil', lambda *a, **k: pytest.fail('a dense wide-map 3x3 ran'))
    with torch.no_grad():
        m(img)
    assert len(grouped) == 33 and all(g == 32 for _, g, _ in grouped)
    assert [(s, st) for s, _, st in grouped if st == 2] == [((2, 256, 10, 14), 2), ((2, 512, 5, 7), 2), ((2, 1024, 3, 4), 2)]
    assert [s[1] for s, _, _ in grouped] == [128] * 3 + [256] * 4 + [512] * 23 + [1024] * 3


def test_chain_from_the_image_to_results(golden_dir):
    """``build_detector`` on the reference's whole x101-32x4d Mask R-CNN config, seeded weights, a 64 x 96 image."""
    import backbone_inputs as bi
    import c4_inputs as ci
    import fpn_inputs as fi
    import resnext_inputs as xi
    import rpn_inputs as ri
    from dynamask_amd import backbones, build_detector
    with open(os.path.join(golden_dir, xi.CONFIGS)) as f:
        cfg = json.load(f)['mask_rcnn_x101_32x4d']
    cfg['test_cfg']['rpn'].update(nms_post=24)
    det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    assert type(det.backbone) is backbones.ResNeXt
    own = det.state_dict()
    state = {}
    for part, fn, seed in (('backbone', bi.head_state, bi.WEIGHT_SEED), ('neck', fi.head_state, fi.WEIGHT_SEED),
                           ('rpn_head', ri.head_state, 27), ('roi_head', ci.head_state, 27)):
        shapes = {k[len(part) + 1:]: v.shape for k, v in own.items() if k.startswith(part + '.')}
        state.update({f'{part}.{k}': v for k, v in fn(shapes, seed).items()})
    det.load_state_dict(state, strict=False)
    det = det.cuda().eval()
    H, W = 64, 96
    img = bi.inputs(1, H, W, seed=6496).cuda()
    metas = [dict(ori_shape=(H, W, 3), img_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=1.0, flip=False, flip_direction=None)]
    with torch.no_grad():
        stages = det.backbone(img)
        assert [tuple(s.shape) for s in stages] == [(1, 256, 16, 24), (1, 512, 8, 12), (1, 1024, 4, 6), (1, 2048, 2, 3)]
        assert all(bool(torch.isfinite(s).all()) and float(s.std()) > 0 for s in stages)
        bbox_results, segm_results = det.simple_test(img, metas)
        bbox_again, segm_again = det.simple_test(img, metas)
    assert len(bbox_results) == 80 and len(segm_results) == 80
    for b, s, b2, s2 in zip(bbox_results, segm_results, bbox_again, segm_again):
        assert b.ndim == 2 and b.shape[1] == 5 and np.isfinite(b).all() and len(s) == len(b)
        assert all(tuple(np.asarray(mask).shape) == (H, W) for mask in s)
        assert b.tobytes() == b2.tobytes() and len(s) == len(s2)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(s, s2))
