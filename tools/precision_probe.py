"""The bf16x3 mode of the implicit-GEMM convolutions against the exact kernel (profiles/r07_precision.txt).

Per inference shape of conv_igemm: ms per launch in both layouts (a HIP graph of back-to-back launches, bench.py's
timer) and the largest error against float64 (torch on the CPU, over the first RoIs); then the headline call
(_mask_forward(last_stage=1), 512 RoIs, graphed) and simple_test_mask_logits at 100 and 16 detections (bucketed graphs)
in both modes.  The per-shape rows call ops.conv2d with each layout directly, so they ignore the routing table
(ops.BF16X3_ROUTES); the whole-call rows go through it.
  python tools/precision_probe.py [reps]"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from dynamask_amd import conv_precision, ops  # noqa: E402
from dynamask_amd.mask_heads import _Conv  # noqa: E402

dev = torch.device('cuda')
REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3

# (label, source channels, cout, ksize, H, NB, split-K scope)
SHAPES = [
    ('conv3x3 256->256 @14, 512 RoIs', [256], 256, 3, 14, 512, False),
    ('conv3x3 256->256 @14, 100 RoIs (split-K)', [256], 256, 3, 14, 100, True),
    ('conv3x3 256->256 @14, 16 RoIs (split-K)', [256], 256, 3, 14, 16, True),
    ('conv3x3 256->36 @14 (DCN offsets), 512', [256], 36, 3, 14, 512, False),
    ('conv3x3 128->36 @28 (DCN offsets), 512', [128], 36, 3, 28, 512, False),
    ('conv3x3 64->36 @56 (DCN offsets), 256', [64], 36, 3, 56, 256, False),
    ('fuse 1x1 [256,256,2]->256 @14, 512', [256, 256, 2], 256, 1, 14, 512, False),
    ('fuse 1x1 [256,256,2]->256 @14, 100 (split-K)', [256, 256, 2], 256, 1, 14, 100, True),
    ('fuse 1x1 [128,128,2]->128 @28, 512', [128, 128, 2], 128, 1, 28, 512, False),
    ('fuse 1x1 [64,64,2]->64 @56, 256', [64, 64, 2], 64, 1, 56, 256, False),
    ('out 1x1 256->256 @14, 512', [256], 256, 1, 14, 512, False),
    ('out 1x1 128->128 @28, 512', [128], 128, 1, 28, 512, False),
    ('out 1x1 64->30 @56, 256', [64], 30, 1, 56, 256, False),
    ('FCN conv_logits 1x1 256->80 @28, 512', [256], 80, 1, 28, 512, False),
]


def f64_error(srcs, conv, out, n=8):
    x = torch.cat([s[:n].cpu() for s in srcs], 1).double()
    ref = torch.nn.functional.conv2d(x, conv.weight.detach().cpu().double(), conv.bias.detach().cpu().double(),
                                     padding=conv.kernel_size // 2)
    return float((out[:n].cpu().double() - ref).abs().max()), float(ref.abs().max())


def shape_row(label, src_c, cout, k, H, NB, splitk):
    torch.manual_seed(7)
    conv = _Conv(sum(src_c), cout, k).to(dev)
    srcs = [torch.randn(NB, c, H, H, device=dev) for c in src_c]
    res = {}
    for p in ('fp32', 'bf16x3'):
        with torch.no_grad():
            wq = conv.packed(src_c, p)

            def fn():
                if splitk:
                    with ops.splitk_scope():
                        return ops.conv2d(srcs, wq, conv.bias.detach(), cout, k)
                return ops.conv2d(srcs, wq, conv.bias.detach(), cout, k)
            try:
                out = fn()
            except RuntimeError as e:            # no bf16x3 build for this shape (DM_ERR_UNSUPPORTED)
                res[p] = None
                print(f'  ({label}: {p}: {str(e).splitlines()[0]})', flush=True)
                continue
            err, scale = f64_error(srcs, conv, out)
            ms = sorted(bench.time_kernel_graphed(fn) for _ in range(REPS))[REPS // 2]
            res[p] = (ms, err, scale)
    flops = 2.0 * NB * H * H * cout * sum(src_c) * k * k
    e = res['fp32']
    line = f'{label:46s} fp32 {e[0]:.4f} ms ({flops / e[0] * 1e-9:5.0f} TF/s) err {e[1]:.3g}'
    s = res['bf16x3']
    if s is None:
        line += ' | bf16x3: no build (DM_ERR_UNSUPPORTED)'
    else:
        line += (f' | bf16x3 {s[0]:.4f} ms ({flops / s[0] * 1e-9:5.0f} fp32-equivalent TF/s) err {s[1]:.3g}'
                 f' | ratio {s[0] / e[0]:.3f}; scale {e[2]:.3g}; routed: {ops.bf16x3_routed(cout, k, H, H)}')
    print(line, flush=True)


def deconv_row(NB=512, H=14, C=256):
    from dynamask_amd.mask_heads import _Deconv
    torch.manual_seed(9)
    d = _Deconv(C, C).to(dev)
    x = torch.randn(NB, C, H, H, device=dev)
    res = {}
    for p in ('fp32', 'bf16x3'):
        with torch.no_grad():
            wp = ops.pack_deconv_weight(d.weight.detach(), precision=p)

            def fn():
                return ops.deconv2x2(x, wp, d.bias.detach(), C, relu=True)
            out = fn()
            xs = x[:8].cpu().double()
            ref = torch.relu(torch.nn.functional.conv_transpose2d(xs, d.weight.detach().cpu().double(),
                                                                  d.bias.detach().cpu().double(), stride=2))
            err = float((out[:8].cpu().double() - ref).abs().max())
            ms = sorted(bench.time_kernel_graphed(fn) for _ in range(REPS))[REPS // 2]
            res[p] = (ms, err)
    flops = 2.0 * NB * H * H * 4 * C * C
    e, s = res['fp32'], res['bf16x3']
    print(f'{"FCN deconv 2x2/s2 256->256 @14, 512":46s} fp32 {e[0]:.4f} ms ({flops / e[0] * 1e-9:5.0f} TF/s) err {e[1]:.3g}'
          f' | bf16x3 {s[0]:.4f} ms ({flops / s[0] * 1e-9:5.0f} fp32-equivalent TF/s) err {s[1]:.3g} | ratio {s[0] / e[0]:.3f};'
          f' routed: {ops.BF16X3_DECONV_MAX_HW[0] >= H * H}', flush=True)


def whole_calls():
    head, _ = bench.build_head(dev)
    feats_c, rois_c, labels_c = bench.make_inputs(0, dev)
    feats = [f.to(dev) for f in feats_c]
    rois, labels = rois_c.to(dev), labels_c.to(dev)
    for p in ('fp32', 'bf16x3'):
        with conv_precision(p), torch.no_grad():
            def step():
                return head._mask_forward(feats, rois, labels, last_stage=1)
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                step()
            hs = sorted(bench.time_kernel(g.replay, iters=20, warmup=3) for _ in range(REPS))
            print(f'[{p}] headline _mask_forward(last_stage=1), 512 RoIs, graphed: {hs[len(hs) // 2]:.4f} ms '
                  f'(all: {", ".join(f"{v:.4f}" for v in hs)})', flush=True)
            del g
            for nd in (100, 16):
                det, dl = rois[:nd, 1:].contiguous(), labels[:nd].contiguous()
                head.enable_inference_graphs(True)

                def call():
                    return head.simple_test_mask_logits(feats, det, dl)
                gr = sorted(bench.time_kernel_median(call, iters=15, warmup=3) for _ in range(REPS))
                head.enable_inference_graphs(False)
                print(f'[{p}] simple_test_mask_logits, {nd} detections, graphed: {gr[len(gr) // 2]:.4f} ms '
                      f'(all: {", ".join(f"{v:.4f}" for v in gr)})', flush=True)


if __name__ == '__main__':
    print(f'# bf16x3 vs exact fp32 convolutions: tools/precision_probe.py, median of {REPS}; err = max |out - float64| '
          f'over the first 8 RoIs', flush=True)
    for s in SHAPES:
        shape_row(*s)
    sem = [(256, 256, 50, 84), (256, 128, 100, 168), (256, 64, 200, 336)]
    torch.manual_seed(8)
    convs = [_Conv(ci, co, 1).to(dev) for ci, co, _, _ in sem]
    xs = [torch.randn(1, ci, h, w, device=dev) for ci, _, h, w in sem]
    for p in ('fp32', 'bf16x3'):
        with torch.no_grad():
            wqs = [c.packed([c.in_channels], p) for c in convs]

            def grp():
                return ops.conv1x1_group(xs, wqs, [c.bias.detach() for c in convs], [c.out_channels for c in convs], relu=True)
            ms = sorted(bench.time_kernel_graphed(grp) for _ in range(REPS))[REPS // 2]
            print(f'semantic 1x1 group P4 / P3 / P2 (one launch)   {p} {ms:.4f} ms', flush=True)
    deconv_row()
    whole_calls()
