"""Whole-detector timing on the MI355X at the reference's test shape: decoded 750 x 1250 uint8 images, resized by the test
pipeline to 800 x 1333 and padded to 800 x 1344, for B = 1 and B = 4, with seeded synthetic weights.

    python tools/detector_infer_bench.py [--reps 10] [--warmup 3] [--rounds 3] [--out FILE]

Every step runs in a child process of its own under its own time limit (``--step-timeout`` seconds); a step that fails or
runs out of time ends the run, nothing is started after it.  Reports, one JSON object per line:

  step ``preprocess``: ``detectors.preprocess`` (one ``dm_preprocess_u8_fwd`` launch) beside the same pipeline steps
      composed of torch device operators -- uint8 -> float, ``F.interpolate(bilinear)``, flip, permute, sub, mul, ``F.pad``.
      That is the stock route, with other rounding (not bit-comparable): context, not a reference.
  steps ``dynamask`` and ``mask_rcnn``: ``detect`` (pre-processing + ``simple_test(rescale=True)``) and ``simple_test`` alone
      in ms and img/s for the DynaMask config and the stock Mask R-CNN config of tests/golden/g29_detector_configs.json;
      the parts timed alone on the same inputs -- backbone, neck, RPN (``simple_test_rpn``), RoI head (``simple_test`` /
      ``batch_simple_test`` on the RPN's proposals) -- with their share of the sum; host waits per call.

``test_cfg.rcnn.score_thr`` is set to 0 so that the synthetic weights give ``max_per_img`` = 100 detections per image: the
mask branch runs at the load of a busy image.  Each figure is the median of ``--reps`` calls timed with HIP events (the
call's own device -> host copies inside the window) after ``--warmup`` calls, ``--rounds`` times; min .. max of the rounds'
medians beside the median.  There is no pass / fail threshold."""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SRC_H, SRC_W = 750, 1250            # -> 800 x 1333 at img_scale (1333, 800), padded to 800 x 1344
STEPS = ('preprocess', 'dynamask', 'mask_rcnn')


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


def rounds_of(fn, args):
    ts = [timed(fn, args.reps, args.warmup) for _ in range(args.rounds)]
    return dict(ms=round(statistics.median(ts), 4), ms_min=round(min(ts), 4), ms_max=round(max(ts), 4), rounds=args.rounds)


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


def images(B):
    import torch
    g = torch.Generator().manual_seed(B)
    return [torch.randint(0, 256, (SRC_H, SRC_W, 3), generator=g, dtype=torch.uint8).cuda() for _ in range(B)]


def torch_preprocess(imgs, norm, size, pad):
    """The pipeline's steps as stock torch device operators, image by image, then the collate."""
    import torch
    import torch.nn.functional as F
    mean = torch.tensor(norm['mean'], device='cuda').view(3, 1, 1)
    stdinv = (1.0 / torch.tensor(norm['std'], device='cuda')).view(3, 1, 1)
    out = []
    for im in imgs:
        x = im.permute(2, 0, 1).float()
        if norm['to_rgb']:
            x = x.flip(0)
        x = F.interpolate(x[None], size=size, mode='bilinear', align_corners=False)[0]
        x = (x - mean) * stdinv
        out.append(F.pad(x, (0, pad[1] - size[1], 0, pad[0] - size[0])))
    return torch.stack(out)


def step_preprocess(args, cfgs, report):
    import torch
    from dynamask_amd import detectors
    cfg = cfgs['mask_rcnn']
    p = detectors.parse_test_pipeline(cfg['test_pipeline'])
    for B in (1, 4):
        imgs = images(B)
        kw = dict(img_scale=p['img_scales'][0], size_divisor=p['size_divisor'])
        out, metas = detectors.preprocess(imgs, p['img_norm_cfg'], **kw)
        size, pad = metas[0]['img_shape'][:2], metas[0]['pad_shape'][:2]
        ref = torch_preprocess(imgs, p['img_norm_cfg'], size, pad)
        r = dict(what='preprocess', B=B, source=[SRC_H, SRC_W], out=list(out.shape),
                 max_abs_diff_to_torch=round(float((out - ref).abs().max()), 4))
        ours, theirs = [], []
        for _ in range(args.rounds):            # alternately
            ours.append(timed(lambda: detectors.preprocess(imgs, p['img_norm_cfg'], **kw), args.reps, args.warmup))
            theirs.append(timed(lambda: torch_preprocess(imgs, p['img_norm_cfg'], size, pad), args.reps, args.warmup))
        r.update(ms=round(statistics.median(ours), 4), ms_min=round(min(ours), 4), ms_max=round(max(ours), 4),
                 torch_ms=round(statistics.median(theirs), 4), torch_ms_min=round(min(theirs), 4),
                 torch_ms_max=round(max(theirs), 4), rounds=args.rounds)
        r['gb_per_s_written'] = round(out.numel() * 4 / r['ms'] / 1e6, 1)
        report(**r)


def step_detector(name, args, cfgs, report):
    import torch
    import bench
    from dynamask_amd import build_detector, detectors
    cfg = copy.deepcopy(cfgs[name])
    cfg['test_cfg']['rcnn']['score_thr'] = 0.0
    det = build_detector(cfg['model'], test_cfg=cfg['test_cfg'])
    det.load_state_dict(seeded_state(det), strict=True)
    det = det.cuda().eval()
    p = detectors.parse_test_pipeline(cfg['test_pipeline'])
    for B in (1, 4):
        imgs = images(B)
        tag = dict(config=name, B=B, source=[SRC_H, SRC_W])
        img, metas = detectors.preprocess(imgs, p['img_norm_cfg'], img_scale=p['img_scales'][0], size_divisor=p['size_divisor'])
        stages = det.backbone(img)
        feats = det.neck(stages)
        props = det.rpn_head.simple_test_rpn(feats, metas)
        roi = det.roi_head.simple_test if B == 1 else det.roi_head.batch_simple_test
        res = det.simple_test(img, metas, rescale=True)
        dets = [sum(len(c) for c in (r[0] if isinstance(r, tuple) else r)) for r in ([res] if B == 1 else res)]
        items = [('detect', lambda: det.detect(imgs, cfg['test_pipeline'])),
                 ('simple_test', lambda: det.simple_test(img, metas, rescale=True)),
                 ('part: backbone', lambda: det.backbone(img)),
                 ('part: neck', lambda: det.neck(stages)),
                 ('part: rpn_head.simple_test_rpn', lambda: det.rpn_head.simple_test_rpn(feats, metas)),
                 ('part: roi_head.' + roi.__name__, lambda: roi(feats, props, metas, rescale=True))]
        rows = []
        for what, fn in items:
            r = dict(what=what, **rounds_of(fn, args), host_waits=bench.count_host_syncs(fn))
            if not what.startswith('part'):
                r['img_per_s'] = round(1000.0 * B / r['ms'], 2)
            rows.append(r)
        total = sum(r['ms'] for r in rows if r['what'].startswith('part'))
        for r in rows:
            if r['what'].startswith('part'):
                r['share_of_parts'] = round(r['ms'] / total, 3)
            report(**r, **tag, img=list(img.shape), proposals=[int(q.shape[0]) for q in props], detections=dets)
        report(what='sum of the parts', ms=round(total, 4), **tag)
        del img, stages, feats, props, items
        torch.cuda.empty_cache()


def run_step(step, args):
    import torch
    with open(os.path.join(ROOT, 'tests', 'golden', 'g29_detector_configs.json')) as f:
        cfgs = json.load(f)

    def report(**r):
        print(json.dumps(r), flush=True)

    with torch.no_grad():
        if step == 'preprocess':
            step_preprocess(args, cfgs, report)
        else:
            step_detector(step, args, cfgs, report)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--step', default=None, choices=STEPS, help='run this one step in this process (what the parent starts)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.step is not None:
        return run_step(args.step, args)
    lines = []
    for step in STEPS:              # the parent never touches the GPU: one fresh child per step, each under its own limit
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--step', step,
               '--reps', str(args.reps), '--warmup', str(args.warmup), '--rounds', str(args.rounds)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, cwd=ROOT)
        sys.stdout.write(p.stdout)
        sys.stdout.flush()
        lines += [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
        if p.returncode != 0:
            sys.exit(f'step {step} ended with status {p.returncode}: nothing more is started')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
