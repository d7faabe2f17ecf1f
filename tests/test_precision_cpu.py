"""The convolution-precision switch (dynamask_amd/precision.py) on the host: no GPU needed."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_default_is_fp32_and_the_context_manager_restores():
    import dynamask_amd as dm
    assert dm.get_conv_precision() == 'fp32'
    with dm.conv_precision('bf16x3') as c:
        assert dm.get_conv_precision() == 'bf16x3'
        with dm.conv_precision('fp32'):
            assert dm.get_conv_precision() == 'fp32'
        assert dm.get_conv_precision() == 'bf16x3'
    assert dm.get_conv_precision() == 'fp32' and c.prev == 'fp32'
    try:
        with dm.conv_precision('bf16x3'):
            raise KeyError('inside')
    except KeyError:
        pass
    assert dm.get_conv_precision() == 'fp32'
    dm.set_conv_precision('bf16x3')
    try:
        assert dm.get_conv_precision() == 'bf16x3'
    finally:
        dm.set_conv_precision('fp32')


@pytest.mark.parametrize('bad', ['bf16', 'FP32', 'tf32', '', None])
def test_unknown_values_raise(bad):
    import dynamask_amd as dm
    with pytest.raises(ValueError):
        dm.set_conv_precision(bad)
    with pytest.raises(ValueError):
        dm.conv_precision(bad)
    assert dm.get_conv_precision() == 'fp32'


def _in_child(code, value):
    env = dict(os.environ, DM_CONV_PRECISION=value, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, '-c', code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_environment_variable_is_read_at_import():
    r = _in_child('import dynamask_amd as d; print(d.get_conv_precision())', 'bf16x3')
    assert r.returncode == 0 and r.stdout.strip() == 'bf16x3', r.stderr
    r = _in_child('import dynamask_amd', 'half')
    assert r.returncode != 0 and 'ValueError' in r.stderr


def test_symbols_exported_and_abi():
    from dynamask_amd import _lib, hazard
    assert _lib.ABI_VERSION == 29
    for name in ('dm_conv_pack_weight_bf16x3', 'dm_conv_packed_floats_bf16x3'):
        assert name in _lib.SIGNATURES
    roles = hazard.parse_header()
    assert roles['dm_conv_pack_weight_bf16x3'][0] == 'in' and roles['dm_conv_pack_weight_bf16x3'][7] == 'out'
    header = open(os.path.join(ROOT, 'include', 'dynamask_hip.h')).read()
    assert '28: the opt-in bf16x3 mode' in header and '#define DM_ABI_VERSION 29' in header
    src = open(os.path.join(ROOT, 'dynamask_amd', 'csrc', 'api_misc.hip')).read()
    assert 'dm_abi_version(void) { return DM_ABI_VERSION; }' in src


def test_mode_applies_only_without_grad_and_outside_the_training_path():
    import dynamask_amd as dm
    from dynamask_amd import ops
    with dm.conv_precision('bf16x3'):
        assert ops.inference_precision() == 'fp32'                     # grad enabled
        with torch.no_grad():
            assert ops.inference_precision() == 'bf16x3'
            assert ops.conv_precision_for(256, 3, 14, 14) == 'bf16x3'
            assert ops.conv_precision_for(36, 3, 14, 14) == 'bf16x3'
            assert ops.conv_precision_for(36, 3, 56, 56) == 'fp32'           # (no bf16x3 build at 56 x 56)
            assert ops.conv_precision_for(30, 1, 56, 56) == 'fp32'           # measured slower
            assert ops.conv_precision_for(128, 1, 28, 28) == 'fp32'
            assert ops.conv_precision_for(80, 1, 28, 28) == 'bf16x3'          # FCNMaskHead conv_logits
            # 3x3: routed only where the kernel has a build (staged plane <= 256 positions)
            assert not any(ops.bf16x3_routed(256, 3, s, s) for s in range(1, 7))
            assert not ops.bf16x3_routed(256, 3, 8, 32) and not ops.bf16x3_routed(256, 3, 1, 200)
            assert all(ops.bf16x3_routed(256, 3, s, s) for s in range(10, 17))
            assert ops.exact_convs(ops.inference_precision)() == 'fp32'      # training path's Functions
            assert ops.inference_precision() == 'bf16x3'
    with torch.no_grad():
        assert ops.conv_precision_for(256, 3, 14, 14) == 'fp32'              # default mode


def test_mask_pre_convs_are_exact():
    import dynamask_amd as dm
    from dynamask_amd.roi_head import MaskPre
    mp = MaskPre()
    with dm.conv_precision('bf16x3'), torch.no_grad():
        assert mp.conv1.precision_for(14, 14) == 'fp32' and mp.conv2.precision_for(28, 28) == 'fp32'


def test_graph_key_differs_between_the_modes(monkeypatch):
    import dynamask_amd as dm
    from dynamask_amd import graphs

    class Head:
        mask_head = torch.nn.Conv2d(2, 2, 1)
    monkeypatch.setattr(torch.cuda, 'current_device', lambda: 0)
    g = graphs.GraphedMaskLogits(Head())
    x = [torch.zeros(1, 2, 4, 4)]
    k32 = g._key(16, x)
    with dm.conv_precision('bf16x3'):
        k3 = g._key(16, x)
    assert k32 != k3 and k32 == g._key(16, x)
