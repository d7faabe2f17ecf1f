"""ResNet-50 backbone timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800, the
Mask R-CNN backbone (``style='pytorch'``, four stages), for B = 1 and B = 4.  Each figure is the median of ``--reps`` calls
timed with HIP events after ``--warmup`` calls; ours and the same layers of tools/stock_backbone.py (stock torch.nn modules
in fp32, whatever kernels torch picks: context, not a reference) are timed alternately, ``--rounds`` times each, and the
min .. max of the rounds' medians is reported beside the median.

    python tools/backbone_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Reports (one JSON object per line): the stem convolution (conv1 + bn1 + ReLU) and the max-pool each alone, every stage,
and ``ResNet.forward``; for the rows that are convolutions, the TFLOP/s and their share of the 157.3 TFLOP/s fp32 matrix
peak.  ``--style caffe`` times the caffe form of the stages instead.  There is no pass / fail
threshold."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

PAD_H, PAD_W = 800, 1344
PEAK_TFLOPS = 157.3
BLOCKS = (3, 4, 6, 3)


def timed(fn, reps, warmup):
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


def build(style):
    from dynamask_amd import backbones
    m = backbones.ResNet(depth=50, style=style)
    g = torch.Generator().manual_seed(1)
    state = {}
    for k, v in m.state_dict().items():          # the recipe of tests/golden/backbone_inputs.head_state: every layer alive
        if k.endswith('num_batches_tracked'):
            state[k] = v
        elif v.dim() == 4:
            state[k] = torch.randn(v.shape, generator=g) * (2.0 / v[0].numel()) ** 0.5
        elif k.endswith('running_var'):
            state[k] = torch.rand(v.shape, generator=g) + 0.5
        elif k.endswith('.weight'):
            state[k] = (torch.rand(v.shape, generator=g) + 0.5) * (0.3 if '.bn3.' in k else 1.0)
        else:
            state[k] = torch.randn(v.shape, generator=g) * 0.1
    m.load_state_dict(state, strict=True)
    return m.cuda().eval()


def build_stock(m):
    """tools/stock_backbone.py's stem and stages with our weights (its blocks put the stride into the 3x3: 'pytorch')."""
    from stock_backbone import ResNet50FPN
    s = ResNet50FPN()
    ours = m.state_dict()
    names = {'c1': 'conv1', 'b1': 'bn1', 'c2': 'conv2', 'b2': 'bn2', 'c3': 'conv3', 'b3': 'bn3', 'down': 'downsample'}
    sd = s.state_dict()
    for k in sd:
        if k.startswith('stem.'):
            src = ('conv1.' if k.startswith('stem.0.') else 'bn1.') + k.split('.', 2)[2]
        elif k.startswith('layers.'):
            _, i, j, part, rest = k.split('.', 4)
            src = f'layer{int(i) + 1}.{j}.{names[part]}.{rest}'
        else:
            continue
        sd[k] = ours[src]
    s.load_state_dict(sd)
    return s.cuda().eval()


def stage_flops(i, B, h, w, stride):
    """Multiply-adds x 2 of stage i on an h x w input ('pytorch': conv1 of block 0 at full size)."""
    planes, cin = 64 * 2 ** i, 64 if i == 0 else 128 * 2 ** i
    ho, wo = -(-h // stride), -(-w // stride)
    f = cin * planes * h * w + 9 * planes * planes * ho * wo + (planes + cin) * 4 * planes * ho * wo
    f += (BLOCKS[i] - 1) * (4 * planes * planes + 9 * planes * planes + planes * 4 * planes) * ho * wo
    return 2.0 * B * f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--style', default='pytorch', choices=('pytorch', 'caffe'))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import ops
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        m = build(args.style)
        stock = build_stock(m) if args.style == 'pytorch' else None
        w7, b7 = m._stem.packed()
        for B in (1, 4):
            tag = dict(B=B, image='1333x800', style=args.style)
            img = torch.randn(B, 3, PAD_H, PAD_W, device='cuda', generator=torch.Generator(device='cuda').manual_seed(B))
            c1 = ops.conv7x7_s2(img, w7, b7, 64, relu=True)
            ins = [ops.maxpool3x3_s2(c1)]
            for i in range(3):
                ins.append(m.run_stage(i, ins[i]))

            def stock_forward():
                x = stock.stem(img)
                for layer in stock.layers:
                    x = layer(x)
                return x
            items = [('stem: conv7x7_s2 (conv1 + bn1 + ReLU)', lambda: ops.conv7x7_s2(img, w7, b7, 64, relu=True),
                      (lambda: stock.stem[:3](img)) if stock else None, 2.0 * B * 147 * 64 * c1.shape[2] * c1.shape[3], list(img.shape)),
                     ('stem: maxpool3x3_s2', lambda: ops.maxpool3x3_s2(c1), (lambda: stock.stem[3](c1)) if stock else None, None,
                      list(c1.shape))]
            for i in range(4):
                x = ins[i]
                items.append((f'layer{i + 1} ({BLOCKS[i]} blocks)', lambda i=i, x=x: m.run_stage(i, x),
                              (lambda i=i, x=x: stock.layers[i](x)) if stock else None,
                              stage_flops(i, B, x.shape[2], x.shape[3], m.strides[i]), list(x.shape)))
            total = items[0][3] + sum(it[3] for it in items[2:])
            items.append(('ResNet.forward', lambda: m(img), stock_forward if stock else None, total, list(img.shape)))
            for what, ours, theirs, flops, shape in items:
                tt = {'ours': [], 'stock': []}
                for _ in range(args.rounds):
                    tt['ours'].append(timed(ours, args.reps, args.warmup))
                    if theirs is not None:
                        tt['stock'].append(timed(theirs, args.reps, args.warmup))
                r = dict(what=what, shape=shape, ms=round(statistics.median(tt['ours']), 4), ms_min=round(min(tt['ours']), 4),
                         ms_max=round(max(tt['ours']), 4), rounds=args.rounds)
                if flops is not None:
                    r['tflops'] = round(flops / r['ms'] / 1e9, 2)
                    r['peak_share'] = round(r['tflops'] / PEAK_TFLOPS, 3)
                if theirs is not None:
                    r.update(stock_ms=round(statistics.median(tt['stock']), 4), stock_ms_min=round(min(tt['stock']), 4),
                             stock_ms_max=round(max(tt['stock']), 4))
                report(**r, **tag)
            del img, c1, ins, items
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
