"""FPN neck timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800 -- the Mask R-CNN
neck, stages C2 256 x 200 x 336, C3 512 x 100 x 168, C4 1024 x 50 x 84, C5 2048 x 25 x 42, five maps of 256 channels out,
for B = 1 and B = 4.  Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls; the
fused and the composed top-down chain are timed alternately, ``--rounds`` times each, and the spread of the rounds' medians
is reported beside them.

    python tools/fpn_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Reports (one JSON object per line): every launch of the fused forward alone (the top lateral, the three merged laterals
``conv2d_up_add``, the four level convolutions, ``subsample2``) with the TFLOP/s of the convolutions, and beside every
merged lateral its composed form (``ops.conv2d`` then ``lat += F.interpolate``); the top-down chain (all four laterals)
fused and composed (``DM_FPN_FUSED=0``) with min / median / max over the rounds, after checking that both paths give the
same bits for every output of the forward; the whole ``FPN.forward``; and a stock ``torch.nn`` FPN in fp32 on the same
stages, as context.  There is no pass / fail threshold."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAD_H, PAD_W = 800, 1344
IN_CHANNELS = [256, 512, 1024, 2048]
STRIDES = [4, 8, 16, 32]


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


def build():
    from dynamask_amd import necks
    m = necks.FPN(IN_CHANNELS, 256, 5)
    g = torch.Generator().manual_seed(1)
    for c in list(m.lateral_convs) + list(m.fpn_convs):
        fan_in = c.conv.weight[0].numel()
        c.conv.weight.data.copy_(torch.randn(c.conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
        c.conv.bias.data.copy_(torch.randn(c.conv.bias.shape, generator=g) * 0.1)
    return m.cuda().eval()


class StockFPN(nn.Module):
    """The same neck of stock torch.nn modules (fp32, whatever kernels torch picks): context, not a reference."""

    def __init__(self, m):
        super().__init__()
        self.lat = nn.ModuleList(nn.Conv2d(c, 256, 1) for c in IN_CHANNELS)
        self.out = nn.ModuleList(nn.Conv2d(256, 256, 3, padding=1) for _ in IN_CHANNELS)
        for mine, theirs in zip(list(self.lat) + list(self.out), list(m.lateral_convs) + list(m.fpn_convs)):
            mine.weight.data.copy_(theirs.conv.weight.data)
            mine.bias.data.copy_(theirs.conv.bias.data)

    def forward(self, xs):
        lats = [c(x) for c, x in zip(self.lat, xs)]
        for i in range(len(lats) - 1, 0, -1):
            lats[i - 1] += F.interpolate(lats[i], size=lats[i - 1].shape[2:], mode='nearest')
        outs = [c(lat) for c, lat in zip(self.out, lats)]
        outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return tuple(outs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from dynamask_amd import necks, ops
    rows = []

    def report(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    def t(fn):
        return round(timed(fn, args.reps, args.warmup), 4)

    with torch.no_grad():
        m = build()
        stock = StockFPN(m).cuda().eval()
        for B in (1, 4):
            tag = dict(B=B, image='1333x800')
            xs = [torch.randn(B, c, -(-PAD_H // s), -(-PAD_W // s), device='cuda',
                              generator=torch.Generator(device='cuda').manual_seed(l))
                  for l, (c, s) in enumerate(zip(IN_CHANNELS, STRIDES))]

            def forward(fused):
                necks.FPN_FUSED[0] = fused
                try:
                    return m(xs)
                finally:
                    necks.FPN_FUSED[0] = True
            a, c = forward(True), forward(False)
            same = all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, c))

            # ---- every launch alone
            convs = [l.conv for l in m.lateral_convs]
            packed = [cv.packed([cv.in_channels]) for cv in convs]
            bias = [cv.bias.detach() for cv in convs]

            def flops(x, cin, k):
                return 2.0 * x.shape[0] * x.shape[2] * x.shape[3] * cin * 256 * k * k

            def conv_row(what, fn, x, cin, k, **kw):
                ms = t(fn)
                report(what=what, ms=ms, tflops=round(flops(x, cin, k) / ms / 1e9, 2), shape=list(x.shape), **kw, **tag)

            conv_row('lateral 3 (C5, top): conv2d 1x1', lambda: convs[3].run(xs[3]), xs[3], 2048, 1)
            lats = [None, None, None, convs[3].run(xs[3])]
            for i in (2, 1, 0):
                iy, ix = m._tables(lats[i + 1], xs[i])
                up = lats[i + 1]
                conv_row(f'lateral {i}: conv2d_up_add', lambda: ops.conv2d_up_add(xs[i], packed[i], bias[i], 256, up, iy, ix),
                         xs[i], IN_CHANNELS[i], 1)
                conv_row(f'lateral {i}: conv2d 1x1 alone', lambda: convs[i].run(xs[i]), xs[i], IN_CHANNELS[i], 1)
                lat = convs[i].run(xs[i])
                report(what=f'lateral {i}: lat += F.interpolate(up) alone', shape=list(lat.shape), **tag,
                       ms=t(lambda: lat.add_(F.interpolate(up, size=lat.shape[2:], mode='nearest'))))
                lats[i] = ops.conv2d_up_add(xs[i], packed[i], bias[i], 256, up, iy, ix)
            for i in range(4):
                kind = 'conv3x3_dil' if lats[i].shape[3] > necks.CONV2D_3X3_MAX_WIDTH else 'conv2d 3x3'
                conv_row(f'level {i}: {kind}', lambda: m._conv3x3(m.fpn_convs[i], lats[i]), lats[i], 256, 3)
            p5 = m._conv3x3(m.fpn_convs[3], lats[3])
            report(what='level 4: subsample2', ms=t(lambda: ops.subsample2(p5)), shape=list(p5.shape), **tag)

            # ---- the top-down chain: fused against composed, alternately
            def chain(fused):
                top = convs[3].run(xs[3])
                for i in (2, 1, 0):
                    if fused:
                        iy, ix = m._tables(top, xs[i])
                        top = ops.conv2d_up_add(xs[i], packed[i], bias[i], 256, top, iy, ix)
                    else:
                        lat = convs[i].run(xs[i])
                        lat += F.interpolate(top, size=lat.shape[2:], mode='nearest')
                        top = lat
                return top
            same_chain = torch.equal(chain(True).view(torch.int32), chain(False).view(torch.int32))
            tt = {True: [], False: []}
            for _ in range(args.rounds):
                for fused in (True, False):
                    tt[fused].append(timed(lambda: chain(fused), args.reps, args.warmup))
            for fused, name in ((True, 'top-down chain, fused'), (False, 'top-down chain, composed (DM_FPN_FUSED=0)')):
                report(what=name, same_bits=same and same_chain, ms=round(statistics.median(tt[fused]), 4),
                       ms_min=round(min(tt[fused]), 4), ms_max=round(max(tt[fused]), 4), rounds=args.rounds, **tag)
            report(what='FPN.forward', ms=t(lambda: forward(True)), same_bits=same, **tag)
            report(what='FPN.forward, composed (DM_FPN_FUSED=0)', ms=t(lambda: forward(False)), **tag)
            report(what='stock torch.nn FPN, fp32 (context)', ms=t(lambda: stock(xs)), **tag)
            del xs, lats, a, c, p5
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, 'w') as f:
            for r in rows:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
