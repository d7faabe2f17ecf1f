"""ResNeXt timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800, B = 1 and B = 4.

    python tools/resnext_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Every step runs in a child process of its own under its own time limit (``--step-timeout`` seconds); a step that fails or
runs out of time ends the run, nothing is started after it.  Reports, one JSON object per line:

  step ``kernel``: per conv2 shape of x101-32x4d and x101-64x4d (the maps 200 x 336 down to 25 x 42, both strides where
      they occur) the grouped launch ``ops.conv3x3_grouped`` (dm_conv3x3_grouped_fwd), its algorithmic bytes
      4 (NB C H W + NB C Ho Wo + 9 C C / groups) over the time as a share of the 8 TB/s HBM peak and of the 6.29 TB/s a
      float4 copy measures, beside the DENSE 3x3 of the same C -> C on the same map on the kernels a
      ResNet stage runs (``ops.conv2d``, ``ops.conv3x3_dil`` on maps wider than layers.CONV2D_3X3_MAX_WIDTH,
      ``ops.conv3x3_s2(splits=1)``: ``groups`` times the arithmetic) and stock ``torch.nn.Conv2d(groups=)`` in fp32 on the
      device (whatever kernel torch picks: context, not a reference).  ``grouped_faster_than_dense``: the grouped launch's
      slowest round is faster than the dense launch's fastest round.
  step ``modules``: ``ResNeXt.forward`` for x101-32x4d and x101-64x4d beside the same layers as stock torch.nn modules
      (defined here) with the same weights.
  step ``detector``: ``MaskRCNN.simple_test`` with the x101-32x4d backbone (tests/golden/g30_resnext_configs.json) beside
      the same detector on ResNet-101, seeded synthetic weights, ``score_thr`` 0 (100 detections per image).

Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls; the launches compared are
timed alternately, ``--rounds`` times each, and the min .. max of the rounds' medians is reported beside the median.  There
is no pass / fail threshold."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAD_H, PAD_W = 800, 1344
SRC_H, SRC_W = 750, 1250            # -> 800 x 1333 at img_scale (1333, 800), padded to 800 x 1344
HBM_PEAK, COPY_PEAK = 8.0e12, 6.29e12
STEPS = ('kernel', 'modules', 'detector')
NETS = {'x101_32x4d': dict(groups=32, base_width=4), 'x101_64x4d': dict(groups=64, base_width=4)}
BLOCKS = (3, 4, 23, 3)


def timed(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def alternately(fns, args):
    """{name: dict(ms, ms_min, ms_max)} of the callables timed in turn, ``--rounds`` times each."""
    ts = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ts[k].append(timed(fn, args.reps, args.warmup))
    return {k: dict(ms=round(statistics.median(v), 4), ms_min=round(min(v), 4), ms_max=round(max(v), 4)) for k, v in ts.items()}


def seeded_state(model, seed=1):
    """Every layer alive: He-scaled weights, norm weights around 1 (0.3 in a block's last norm), small biases and running
    means, running variances in [0.5, 1.5]."""
    import torch
    g = torch.Generator().manual_seed(seed)
    state = {}
    for k, v in model.state_dict().items():
        if k.endswith('num_batches_tracked'):
            state[k] = v
        elif k.endswith('running_var'):
            state[k] = torch.rand(v.shape, generator=g) + 0.5
        elif v.dim() > 1:
            state[k] = torch.randn(v.shape, generator=g) * (2.0 / max(v[0].numel(), 1)) ** 0.5
        elif k.endswith('.weight'):
            state[k] = (torch.rand(v.shape, generator=g) + 0.5) * (0.3 if '.bn3.' in k else 1.0)
        else:
            state[k] = torch.randn(v.shape, generator=g) * 0.1
    return state


def conv2_shapes(groups, base_width):
    """(layer, C, H, W, stride) of every distinct conv2 launch of an x101 net on the padded image ('pytorch' style)."""
    h, w = PAD_H // 4, PAD_W // 4
    out = []
    for i in range(4):
        C = (64 * 2 ** i * base_width // 64) * groups
        if i > 0:
            out.append((f'layer{i + 1}.0', C, h, w, 2))
            h, w = (h + 1) // 2, (w + 1) // 2
        out.append((f'layer{i + 1}.{1 if i else 0}+', C, h, w, 1))
    return out


# ------------------------------------------------------------------------------------------------ the kernel
def step_kernel(args, report):
    import torch
    from dynamask_amd import layers, ops
    for net, kw in NETS.items():
        groups = kw['groups']
        for B in (1, 4):
            for where, C, H, W, stride in conv2_shapes(**kw):
                g = torch.Generator(device='cuda').manual_seed(C + H + stride)
                x = torch.randn(B, C, H, W, device='cuda', generator=g)
                w = torch.randn(C, C // groups, 3, 3, device='cuda', generator=g) * (2.0 / (9 * C // groups)) ** 0.5
                wd = torch.randn(C, C, 3, 3, device='cuda', generator=g) * (2.0 / (9 * C)) ** 0.5
                b = torch.randn(C, device='cuda', generator=g) * 0.1
                wq, wdq = ops.pack_grouped_conv_weight(w, groups), ops.pack_conv_weight(wd, src_channels=[C])
                stock = torch.nn.Conv2d(C, C, 3, stride, 1, groups=groups).cuda()
                stock.weight.copy_(w)
                stock.bias.copy_(b)
                if stride == 2:
                    dense_name, dense = 'ops.conv3x3_s2(splits=1)', lambda: ops.conv3x3_s2(x, wdq, b, C, relu=True, splits=1)
                elif W > layers.CONV2D_3X3_MAX_WIDTH:
                    dense_name, dense = 'ops.conv3x3_dil', lambda: ops.conv3x3_dil(x, wdq, b, C, 1, relu=True)
                else:
                    dense_name, dense = 'ops.conv2d', lambda: ops.conv2d(x, wdq, b, C, 3, relu=True)
                fns = {'grouped': lambda: ops.conv3x3_grouped(x, wq, b, groups, stride=stride, relu=True), 'dense': dense,
                       'stock': lambda: torch.relu(stock(x))}
                try:
                    dense()
                except RuntimeError as e:       # a shape the dense kernel refuses: said in the row, the rest is timed
                    dense_name += f' refused: {e}'
                    del fns['dense']
                t = alternately(fns, args)
                t.setdefault('dense', dict(ms=None, ms_min=None, ms_max=None))
                Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
                nbytes = 4 * (B * C * H * W + B * C * Ho * Wo + 9 * C * C // groups)
                r = dict(what='conv2', net=net, where=where, B=B, C=C, groups=groups, per_group=C // groups, map=[H, W], stride=stride,
                         rounds=args.rounds, **t['grouped'], mbytes=round(nbytes / 1e6, 2),
                         hbm_peak_share=round(nbytes / (t['grouped']['ms'] * 1e-3) / HBM_PEAK, 3),
                         copy_peak_share=round(nbytes / (t['grouped']['ms'] * 1e-3) / COPY_PEAK, 3),
                         gflops=round(2.0 * 9 * B * C * (C // groups) * Ho * Wo / 1e9, 2), dense=dense_name,
                         **{f'dense_{k}': v for k, v in t['dense'].items()}, **{f'stock_{k}': v for k, v in t['stock'].items()},
                         grouped_faster_than_dense=None if t['dense']['ms'] is None else t['grouped']['ms_max'] < t['dense']['ms_min'])
                report(**r)
                del x, w, wd, wq, wdq, stock
            torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the modules
def stock_resnext(groups, base_width):
    """The same layers as stock torch.nn modules, BatchNorm in eval mode ('pytorch' style, depth 101)."""
    import torch.nn as nn
    import torch.nn.functional as F

    class Block(nn.Module):
        def __init__(self, cin, planes, stride):
            super().__init__()
            width, cout = (planes * base_width // 64) * groups, planes * 4
            self.conv1, self.bn1 = nn.Conv2d(cin, width, 1, bias=False), nn.BatchNorm2d(width)
            self.conv2, self.bn2 = nn.Conv2d(width, width, 3, stride, 1, groups=groups, bias=False), nn.BatchNorm2d(width)
            self.conv3, self.bn3 = nn.Conv2d(width, cout, 1, bias=False), nn.BatchNorm2d(cout)
            self.downsample = None
            if stride != 1 or cin != cout:
                self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

        def forward(self, x):
            idt = x if self.downsample is None else self.downsample(x)
            x = F.relu(self.bn1(self.conv1(x)))
            x = F.relu(self.bn2(self.conv2(x)))
            return F.relu(self.bn3(self.conv3(x)) + idt)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
            cin = 64
            for i, n in enumerate(BLOCKS):
                blocks = []
                for j in range(n):
                    blocks.append(Block(cin, 64 * 2 ** i, 2 if (j == 0 and i > 0) else 1))
                    cin = 256 * 2 ** i
                setattr(self, f'layer{i + 1}', nn.Sequential(*blocks))

        def forward(self, img):
            x = F.max_pool2d(F.relu(self.bn1(self.conv1(img))), 3, 2, 1)
            outs = []
            for i in range(4):
                x = getattr(self, f'layer{i + 1}')(x)
                outs.append(x)
            return tuple(outs)
    return Net()


def step_modules(args, report):
    import torch
    import bench
    from dynamask_amd import backbones
    for net, kw in NETS.items():
        m = backbones.ResNeXt(depth=101, **kw)
        state = seeded_state(m)
        m.load_state_dict(state, strict=True)
        m = m.cuda().eval()
        stock = stock_resnext(**kw)
        stock.load_state_dict(state, strict=True)          # the reference's keys are torch's own
        stock = stock.cuda().eval()
        for B in (1, 4):
            img = torch.randn(B, 3, PAD_H, PAD_W, device='cuda', generator=torch.Generator(device='cuda').manual_seed(B))
            ours, theirs = m(img), stock(img)
            diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, theirs))
            t = alternately({'ours': lambda: m(img), 'stock': lambda: stock(img)}, args)
            report(what='ResNeXt.forward', net=net, B=B, image=[PAD_H, PAD_W], rounds=args.rounds, **t['ours'],
                   img_per_s=round(1000.0 * B / t['ours']['ms'], 2), **{f'stock_{k}': v for k, v in t['stock'].items()},
                   max_rel_diff_to_stock=round(diff, 7), host_waits=bench.count_host_syncs(lambda: m(img)))
            del img, ours, theirs
            torch.cuda.empty_cache()
        del m, stock
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the detector
def step_detector(args, report, fixture='g30_resnext_configs.json', entry='mask_rcnn_x101_32x4d'):
    """``fixture`` / ``entry``: the detector config timed beside ResNet-101 (tools/res2net_infer_bench.py passes its own)."""
    import torch
    import bench
    from dynamask_amd import build_detector, detectors
    golden = os.path.join(ROOT, 'tests', 'golden')
    with open(os.path.join(golden, 'g29_detector_configs.json')) as f:
        r50 = json.load(f)['mask_rcnn']
    with open(os.path.join(golden, fixture)) as f:
        x101 = json.load(f)[entry]
    r101 = copy.deepcopy(r50)
    r101['model']['backbone']['depth'] = 101
    p = detectors.parse_test_pipeline(r50['test_pipeline'])
    for name, cfg in ((entry, x101), ('mask_rcnn_r101', r101)):
        cfg = copy.deepcopy(cfg)
        cfg['test_cfg']['rcnn']['score_thr'] = 0.0
        det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
        det.load_state_dict(seeded_state(det), strict=True)
        det = det.cuda().eval()
        for B in (1, 4):
            g = torch.Generator().manual_seed(B)
            imgs = [torch.randint(0, 256, (SRC_H, SRC_W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]
            img, metas = detectors.preprocess(imgs, p['img_norm_cfg'], img_scale=p['img_scales'][0], size_divisor=p['size_divisor'])
            res = det.simple_test(img, metas, rescale=True)
            dets = [sum(len(c) for c in (r[0] if isinstance(r, tuple) else r)) for r in ([res] if B == 1 else res)]
            t = alternately({'simple_test': lambda: det.simple_test(img, metas, rescale=True), 'backbone': lambda: det.backbone(img)}, args)
            report(what='MaskRCNN.simple_test', config=name, B=B, img=list(img.shape), rounds=args.rounds, **t['simple_test'],
                   img_per_s=round(1000.0 * B / t['simple_test']['ms'], 2), **{f'backbone_{k}': v for k, v in t['backbone'].items()},
                   detections=dets, host_waits=bench.count_host_syncs(lambda: det.simple_test(img, metas, rescale=True)))
            del img, imgs
            torch.cuda.empty_cache()
        del det
        torch.cuda.empty_cache()


def run_step(step, args, step_fns):
    import torch

    def report(**r):
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        step_fns[step](args, report)


def main(step_fns=None, script=None):
    """``step_fns`` {step: function} and ``script`` (the file a child runs): another tool's steps on this harness
    (tools/res2net_infer_bench.py); the defaults are this tool's."""
    step_fns = step_fns or {'kernel': step_kernel, 'modules': step_modules, 'detector': step_detector}
    script = os.path.abspath(script or __file__)
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--steps', default=','.join(STEPS), help='comma-separated subset of ' + ', '.join(STEPS))
    ap.add_argument('--step', default=None, choices=STEPS, help='run this one step in this process (what the parent starts)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step is not None:
        return run_step(args.step, args, step_fns)
    lines = []
    for step in args.steps.split(','):            # the parent never touches the GPU: one fresh child per step, each under its own limit
        if step not in STEPS:
            sys.exit(f'no step {step!r}: {STEPS}')
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, script, '--step', step,
               '--reps', str(args.reps), '--warmup', str(args.warmup), '--rounds', str(args.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if args.out:
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        if p.returncode != 0:
            sys.exit(f'step {step} ended with status {p.returncode}: nothing more is started')


if __name__ == '__main__':
    main()
