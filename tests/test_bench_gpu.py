"""A plain `bench.py --gpus 1 --steps N --warmup W` does what its headline figure needs and nothing else; everything
beside the headline leg is behind --full (tools/collect_profiles.sh calls it that way)."""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

HEADLINE_KEYS = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step')
FULL_ONLY_KEYS = ('extra', 'roofline', 'roofline_dcn', 'roofline_roialign', 'cpu_baseline', 'entry_points', 'forward_train_ms',
                  'train_ms_per_step', 'allreduce_alone_ms', 'inference_100dets_ms', 'end_to_end_img_per_s', 'backbone_fpn_ms')


def test_plain_run_times_the_headline_leg_alone_within_30_s_outside_its_steps(tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    steps, warmup = 6, 2
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', str(warmup),
                        '--dump-outputs', str(tmp_path / 'd')], env=env, capture_output=True, text=True, timeout=170)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(r.stdout.splitlines()) == 1                      # stdout carries the line and nothing else
    out = json.loads(r.stdout)
    for k in HEADLINE_KEYS:
        assert k in out, k
    assert out['full'] is False and out['steps'] == steps and out['warmup'] == warmup and out['n_gpus'] == 1
    assert out['unit'] == 'img/s' and out['higher_is_better'] is True and out['dtype'] == 'f32'
    assert out['ms_per_step'] > 0 and abs(out['value'] - 1e3 / out['ms_per_step']) < 1e-9 * out['value']
    assert out['config']['launch'] == 'hip graph replay'
    for k in FULL_ONLY_KEYS:
        assert k not in out, k
    assert sorted(os.listdir(tmp_path / 'd')) == sorted(f'{k}_{i}.npy' for k in ('stage_instance_preds', 'stage_detail_preds')
                                                        for i in range(2))
    outside = wall - (steps + warmup) * out['ms_per_step'] * 1e-3
    print(f'plain run: {wall:.2f} s in all, {outside:.2f} s outside its {steps + warmup} steps')
    assert outside <= 30.0
