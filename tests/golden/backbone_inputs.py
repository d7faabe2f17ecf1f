"""Seeded inputs and weights of the backbone fixture (g28_backbone*.npz: the unchanged ``model.backbone`` of the FPN and the
C4 Mask R-CNN configs), shared by tests/golden/make_golden_backbone.py and the tests: the fixture stores outputs only.
``restate`` is a torch restatement of ResNet's forward (BatchNorm NOT folded) from a resolved config and a state_dict, for
machines without the reference; the generator asserts that it gives the reference's outputs bit for bit on the CPU, in
float32 and in float64.

The images are 2 x 3 x 37 x 53: odd sizes, no multiple of 32.  The stem gives 19 x 27 and 10 x 14; C2 is 10 x 14, C3 5 x 7,
C4 3 x 4, C5 2 x 2 -- every stride-2 step but the first meets an even and an odd size."""
import torch
import torch.nn.functional as F

from rpn_inputs import ERR_SCALE, pack_err, unpack_f64  # noqa: F401  (the twins' form is the RPN fixture's)

BATCH, IMG_H, IMG_W = 2, 37, 53
IMG_SEED = 282828
WEIGHT_SEED = 28
STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
# form -> (the config its ``model.backbone`` comes from, the depth-101 config of the same style: built, not run)
FORMS = {'pytorch': ('configs/_base_/models/mask_rcnn_r50_fpn.py', 'configs/mask_rcnn/mask_rcnn_r101_fpn_1x_coco.py'),
         'caffe_c4': ('configs/_base_/models/mask_rcnn_r50_caffe_c4.py', None)}
# one file per form keeps every committed file below 1 MiB
FILES = {'pytorch': 'g28_backbone.npz', 'caffe_c4': 'g28_backbone_caffe_c4.npz'}


def inputs(batch=BATCH, h=IMG_H, w=IMG_W, seed=IMG_SEED):
    """[batch, 3, h, w], image b from seed + b: a batch's image does not depend on the batch."""
    return torch.cat([torch.randn(1, 3, h, w, generator=torch.Generator().manual_seed(seed + b)) for b in range(batch)]).contiguous()


def head_state(shapes, seed=WEIGHT_SEED):
    """Seeded parameters and statistics for ``shapes`` {key: shape} of a ResNet state_dict that keep all its layers alive:
    convolutions N(0, 2 / fan_in); BatchNorm weight U(0.5, 1.5) -- times 0.3 in every ``bn3``, so that the residual sums
    do not grow block by block --, bias and running_mean N(0, 0.1^2), running_var U(0.5, 1.5)."""
    g = torch.Generator().manual_seed(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(shapes[k])
        if k.endswith('num_batches_tracked'):
            out[k] = torch.zeros(shape, dtype=torch.long)
        elif len(shape) == 4:
            fan_in = shape[1] * shape[2] * shape[3]
            out[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith('running_var'):
            out[k] = torch.rand(shape, generator=g) + 0.5
        elif k.endswith('.weight'):
            out[k] = (torch.rand(shape, generator=g) + 0.5) * (0.3 if '.bn3.' in k else 1.0)
        else:               # BatchNorm bias, running_mean
            out[k] = torch.randn(shape, generator=g) * 0.1
    return out


def resolve(backbone):
    """The settings the forward depends on, from a backbone config (``type`` may be present)."""
    cfg = dict(backbone)
    cfg.pop('type', None)
    n = cfg.get('num_stages', 4)
    return dict(blocks=STAGE_BLOCKS[cfg['depth']][:n], strides=tuple(cfg.get('strides', (1, 2, 2, 2)))[:n],
                out_indices=tuple(cfg.get('out_indices', (0, 1, 2, 3))), style=cfg.get('style', 'pytorch'))


def _params(state, like):
    return {k: (v.to(like.dtype) if v.is_floating_point() else v).to(like.device) for k, v in state.items()}


def _bn(x, p, prefix):
    return F.batch_norm(x, p[prefix + '.running_mean'], p[prefix + '.running_var'], p[prefix + '.weight'], p[prefix + '.bias'],
                        False, 0.1, 1e-5)


def restate_stem(state, img):
    """maxpool(relu(bn1(conv1(img))))."""
    p = _params(state, img)
    x = F.relu(_bn(F.conv2d(img, p['conv1.weight'], stride=2, padding=3), p, 'bn1'))
    return F.max_pool2d(x, 3, stride=2, padding=1)


def restate_stage(backbone, state, i, x):
    """Stage ``i`` (``layer{i + 1}``) on its input ``x``, in the reference's order of operations."""
    r = resolve(backbone)
    p = _params(state, x)
    for j in range(r['blocks'][i]):
        pre = f'layer{i + 1}.{j}'
        stride = r['strides'][i] if j == 0 else 1
        s1, s2 = (1, stride) if r['style'] == 'pytorch' else (stride, 1)
        out = F.relu(_bn(F.conv2d(x, p[pre + '.conv1.weight'], stride=s1), p, pre + '.bn1'))
        out = F.relu(_bn(F.conv2d(out, p[pre + '.conv2.weight'], stride=s2, padding=1), p, pre + '.bn2'))
        out = _bn(F.conv2d(out, p[pre + '.conv3.weight']), p, pre + '.bn3')
        identity = x
        if pre + '.downsample.0.weight' in p:
            identity = _bn(F.conv2d(x, p[pre + '.downsample.0.weight'], stride=stride), p, pre + '.downsample.1')
        out += identity
        x = F.relu(out)
    return x


def restate(backbone, state, img, every_stage=False):
    """The backbone's outputs for ``img`` with the parameters ``state`` (keys of ResNet.state_dict), in the dtype and on
    the device of ``img``.  ``every_stage``: (the stem's output, [every stage's output]) instead of the ``out_indices``."""
    r = resolve(backbone)
    stem = restate_stem(state, img)
    x, stages = stem, []
    for i in range(len(r['blocks'])):
        x = restate_stage(backbone, state, i, x)
        stages.append(x)
    if every_stage:
        return stem, stages
    return tuple(stages[i] for i in range(len(stages)) if i in r['out_indices'])
