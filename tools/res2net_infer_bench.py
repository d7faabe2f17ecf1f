"""Res2Net timing on the MI355X at the reference's test shape: a 1333 x 800 image padded to 1344 x 800, B = 1 and B = 4.

    python tools/res2net_infer_bench.py [--reps 20] [--warmup 5] [--rounds 5] [--out FILE]

Every step runs in a child process of its own under its own time limit (``--step-timeout`` seconds); a step that fails or
runs out of time ends the run, nothing is started after it.  Reports, one JSON object per line:

  step ``kernel``: per 3x3 shape of R2-101 (26 / 52 / 104 / 208 channels per scale on the maps 200 x 336 down to
      25 x 42, both block kinds where they occur) what stands where conv2 stood in a block.  ``stage``: ONE
      ``ops.conv3x3_slices`` launch (dm_conv3x3_slices_fwd) with G = 3 and the tail (the copy at stride 1, the 3x3
      average pool at stride 2).  ``normal``: the three launches with G = 1 in a row, the second and third with the
      previous output as addend, the first with the copy as tail.  Beside each the same arithmetic by stock torch in
      fp32 on the device -- ``torch.split``, three ``torch.nn.Conv2d`` on contiguous slices (+ the adds), the tail and
      ``torch.cat``, whatever kernels torch picks: context, not a reference -- and the launch's algorithmic bytes
      4 (read 4 w H W, written 4 w Ho Wo, weights 27 w w; the normal block reads two slices a second time as addends)
      over the time as a share of the 8 TB/s HBM peak.
  step ``modules``: ``Res2Net.forward`` for R2-101 beside the same layers as stock torch.nn modules (defined here) with
      the same weights.
  step ``detector``: ``MaskRCNN.simple_test`` with the R2-101 backbone (tests/golden/g31_res2net_configs.json) beside
      the same detector on ResNet-101, seeded synthetic weights, ``score_thr`` 0 (100 detections per image).

Each figure is the median of ``--reps`` calls timed with HIP events after ``--warmup`` calls; the launches compared are
timed alternately, ``--rounds`` times each, and the min .. max of the rounds' medians is reported beside the median.  There
is no pass / fail threshold."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import resnext_infer_bench  # noqa: E402
from resnext_infer_bench import HBM_PEAK, PAD_H, PAD_W, alternately, main, seeded_state  # noqa: E402

BLOCKS = (3, 4, 23, 3)
SCALES, BASE_WIDTH = 4, 26


def conv_shapes():
    """(layer, kind, w, H, W, stride) of every distinct sliced launch pattern of R2-101 on the padded image."""
    h, w = PAD_H // 4, PAD_W // 4
    out = []
    for i in range(4):
        c = 64 * 2 ** i * BASE_WIDTH // 64
        out.append((f'layer{i + 1}.0', 'stage', c, h, w, 2 if i else 1))
        if i:
            h, w = (h + 1) // 2, (w + 1) // 2
        out.append((f'layer{i + 1}.1+', 'normal', c, h, w, 1))
    return out


# ------------------------------------------------------------------------------------------------ the kernel
def step_kernel(args, report):
    import torch
    import torch.nn.functional as F
    from dynamask_amd import ops
    for B in (1, 4):
        for where, kind, w, H, W, stride in conv_shapes():
            g = torch.Generator(device='cuda').manual_seed(w + H + stride)
            x = torch.randn(B, 4 * w, H, W, device='cuda', generator=g)
            wt = torch.randn(3, w, w, 3, 3, device='cuda', generator=g) * (2.0 / (9 * w)) ** 0.5
            b = torch.randn(3 * w, device='cuda', generator=g) * 0.1
            Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
            cat = torch.empty(B, 4 * w, Ho, Wo, device='cuda')
            stock = [torch.nn.Conv2d(w, w, 3, stride, 1).cuda() for _ in range(3)]
            for i, m in enumerate(stock):
                m.weight.copy_(wt[i])
                m.bias.copy_(b[i * w:(i + 1) * w])
            if kind == 'stage':
                wq = ops.pack_conv_slices_weight(wt)

                def ours():
                    return ops.conv3x3_slices(x, wq, b, w, 3, cat, stride=stride, relu=True, tail=2 if stride == 2 else 1,
                                              tail_x_ch0=3 * w, tail_o_ch0=3 * w)

                def theirs():
                    spx = torch.split(x, w, 1)
                    outs = [torch.relu(stock[i](spx[i].contiguous())) for i in range(3)]
                    outs.append(F.avg_pool2d(spx[3], 3, stride, 1) if stride == 2 else spx[3])
                    return torch.cat(outs, 1)
                reads = 4
            else:
                wqs = [ops.pack_conv_slices_weight(wt[i:i + 1].contiguous()) for i in range(3)]
                bs = [b[i * w:(i + 1) * w].contiguous() for i in range(3)]

                def ours():
                    for i in range(3):
                        ops.conv3x3_slices(x, wqs[i], bs[i], w, 1, cat, relu=True, x_ch0=i * w, o_ch0=i * w, addend=cat if i else None,
                                           a_ch0=(i - 1) * w if i else 0, tail=0 if i else 1, tail_x_ch0=3 * w, tail_o_ch0=3 * w)
                    return cat

                def theirs():
                    spx = torch.split(x, w, 1)
                    sp = torch.relu(stock[0](spx[0].contiguous()))
                    outs = [sp]
                    for i in (1, 2):
                        sp = torch.relu(stock[i]((sp + spx[i]).contiguous()))
                        outs.append(sp)
                    outs.append(spx[3])
                    return torch.cat(outs, 1)
                reads = 6
            diff = float((ours() - theirs()).abs().max() / theirs().abs().max())
            t = alternately({'ours': ours, 'stock': theirs}, args)
            nbytes = 4 * (B * reads * w * H * W + B * 4 * w * Ho * Wo + 27 * w * w)
            report(what='sliced 3x3', where=where, kind=kind, B=B, w=w, map=[H, W], stride=stride, launches=1 if kind == 'stage' else 3,
                   rounds=args.rounds, **t['ours'], mbytes=round(nbytes / 1e6, 2),
                   hbm_peak_share=round(nbytes / (t['ours']['ms'] * 1e-3) / HBM_PEAK, 3),
                   gflops=round(2.0 * 27 * B * w * w * Ho * Wo / 1e9, 2),
                   tflops=round(2.0 * 27 * B * w * w * Ho * Wo / (t['ours']['ms'] * 1e-3) / 1e12, 2),
                   **{f'stock_{k}': v for k, v in t['stock'].items()}, max_rel_diff_to_stock=round(diff, 7))
            del x, wt, cat, stock
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ the modules
def stock_res2net():
    """The same layers as stock torch.nn modules, BatchNorm in eval mode (depth 101, 26w x 4s), keys as the reference's."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    s = SCALES

    class Block(nn.Module):
        def __init__(self, cin, planes, stride, stage):
            super().__init__()
            w, cout = planes * BASE_WIDTH // 64, planes * 4
            self.w, self.stride, self.stage = w, stride, stage
            self.conv1, self.bn1 = nn.Conv2d(cin, w * s, 1, bias=False), nn.BatchNorm2d(w * s)
            self.conv3, self.bn3 = nn.Conv2d(w * s, cout, 1, bias=False), nn.BatchNorm2d(cout)
            self.downsample = None
            if stride != 1 or cin != cout:
                self.downsample = nn.Sequential(nn.AvgPool2d(stride, stride, ceil_mode=True, count_include_pad=False),
                                                nn.Conv2d(cin, cout, 1, bias=False), nn.BatchNorm2d(cout))
            self.convs = nn.ModuleList([nn.Conv2d(w, w, 3, stride, 1, bias=False) for _ in range(s - 1)])
            self.bns = nn.ModuleList([nn.BatchNorm2d(w) for _ in range(s - 1)])

        def forward(self, x):
            idt = x if self.downsample is None else self.downsample(x)
            spx = torch.split(F.relu(self.bn1(self.conv1(x))), self.w, 1)
            sp = F.relu(self.bns[0](self.convs[0](spx[0].contiguous())))
            outs = [sp]
            for i in range(1, s - 1):
                sp = spx[i] if self.stage else sp + spx[i]
                sp = F.relu(self.bns[i](self.convs[i](sp.contiguous())))
                outs.append(sp)
            outs.append(F.avg_pool2d(spx[s - 1], 3, self.stride, 1) if self.stage and self.stride != 1 else spx[s - 1])
            return F.relu(self.bn3(self.conv3(torch.cat(outs, 1))) + idt)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.stem = nn.Sequential(nn.Conv2d(3, 32, 3, 2, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
                                      nn.Conv2d(32, 32, 3, 1, 1, bias=False), nn.BatchNorm2d(32), nn.ReLU(inplace=True),
                                      nn.Conv2d(32, 64, 3, 1, 1, bias=False), nn.BatchNorm2d(64), nn.ReLU(inplace=True))
            cin = 64
            for i, n in enumerate(BLOCKS):
                blocks = []
                for j in range(n):
                    blocks.append(Block(cin, 64 * 2 ** i, 2 if (j == 0 and i > 0) else 1, j == 0))
                    cin = 256 * 2 ** i
                setattr(self, f'layer{i + 1}', nn.Sequential(*blocks))

        def forward(self, img):
            x = F.max_pool2d(self.stem(img), 3, 2, 1)
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
    m = backbones.Res2Net(depth=101, scales=SCALES, base_width=BASE_WIDTH)
    state = seeded_state(m)
    m.load_state_dict(state, strict=True)
    m = m.cuda().eval()
    stock = stock_res2net()
    stock.load_state_dict(state, strict=True)          # the reference's keys are torch's own
    stock = stock.cuda().eval()
    for B in (1, 4):
        img = torch.randn(B, 3, PAD_H, PAD_W, device='cuda', generator=torch.Generator(device='cuda').manual_seed(B))
        ours, theirs = m(img), stock(img)
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ours, theirs))
        t = alternately({'ours': lambda: m(img), 'stock': lambda: stock(img)}, args)
        report(what='Res2Net.forward', net='r2_101', B=B, image=[PAD_H, PAD_W], rounds=args.rounds, **t['ours'],
               img_per_s=round(1000.0 * B / t['ours']['ms'], 2), **{f'stock_{k}': v for k, v in t['stock'].items()},
               max_rel_diff_to_stock=round(diff, 7), host_waits=bench.count_host_syncs(lambda: m(img)))
        del img, ours, theirs
        torch.cuda.empty_cache()


def step_detector(args, report):
    resnext_infer_bench.step_detector(args, report, 'g31_res2net_configs.json', 'mask_rcnn_r2_101')


if __name__ == '__main__':
    main({'kernel': step_kernel, 'modules': step_modules, 'detector': step_detector}, __file__)
