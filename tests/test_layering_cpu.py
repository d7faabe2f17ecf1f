"""The package's layering, without a GPU: ``layers`` and ``postprocess`` import none of the modules built from them, the
neck, the backbone and the shared head import no RoI or dense head, no relative import hides inside a function, importing
``roi_head`` alone fills the registries its configs name, every model section starts from the weights recorded in
tests/golden/module_init_digest.json (tools/module_digest.py), and the one linear holder draws as ``nn.Linear`` /
``xavier_uniform_`` do."""
import ast
import glob
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'dynamask_amd')
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import module_digest  # noqa: E402

SECTIONS = dict(module_digest.sections())

# module -> the modules its import must not load
HEADS_ETC = ('mask_heads', 'bbox_heads', 'roi_head', 'dense_heads', 'necks', 'backbones', 'shared_heads', 'train_path')
FORBIDDEN = {
    'layers': HEADS_ETC,
    'postprocess': HEADS_ETC,
    'backbones': ('roi_head', 'mask_heads', 'bbox_heads', 'dense_heads', 'anchors'),
    'necks': ('roi_head', 'mask_heads', 'bbox_heads', 'dense_heads', 'anchors'),
    'shared_heads': ('bbox_heads', 'roi_head', 'mask_heads'),
}
# the modules whose registrations are checked: the RoI heads' and, for the other model sections, the section's own
REGISTERING = ('roi_head', 'dense_heads', 'necks', 'backbones')

# what a fresh interpreter prints after importing ONE module: the package's loaded modules and every registry's names
CHILD = r'''
import importlib, json, sys
importlib.import_module('dynamask_amd.' + sys.argv[1])
from dynamask_amd.registry import Registry
mods = {n[len('dynamask_amd.'):]: m for n, m in sys.modules.items() if n.startswith('dynamask_amd.') and m is not None}
regs = {}
for m in mods.values():
    for v in vars(m).values():
        if isinstance(v, Registry):
            regs[v.name] = sorted(v.module_dict)
print(json.dumps(dict(modules=sorted(mods), registries=regs)))
'''


@pytest.fixture(scope='module')
def fresh():
    """module -> what CHILD reports; one fresh interpreter per module (``sys.modules`` is shared in-process), all started
    together."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    procs = {m: subprocess.Popen([sys.executable, '-c', CHILD, m], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                                 cwd=ROOT) for m in sorted(set(FORBIDDEN) | set(REGISTERING))}
    out = {}
    for m, p in procs.items():
        so, se = p.communicate()
        assert p.returncode == 0, f'import dynamask_amd.{m} failed:\n{se.decode()}'
        out[m] = json.loads(so.decode().strip().splitlines()[-1])
    return out


# ------------------------------------------------------------------------------------------------ leaves stay leaves
@pytest.mark.parametrize('module', sorted(FORBIDDEN))
def test_import_loads_nothing_above_it(fresh, module):
    loaded = set(fresh[module]['modules'])
    assert module in loaded
    assert not loaded & set(FORBIDDEN[module]), sorted(loaded & set(FORBIDDEN[module]))


# ------------------------------------------------------------------------------------------------ no hidden imports
# (file, enclosing function) of the relative imports that may sit inside a body, each with its reason
LOCAL_IMPORTS_ALLOWED = {
    # the package's lazy attributes (NECKS, FPN, BACKBONES, ResNet ...): ``import dynamask_amd`` alone must not load the
    # operator bindings that necks.py and backbones.py import
    ('__init__.py', '__getattr__'),
}


def test_no_relative_import_inside_a_body():
    found = set()
    for path in sorted(glob.glob(os.path.join(PKG, '*.py'))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for scope in ast.walk(tree):
            if isinstance(scope, (ast.FunctionDef, ast.AsyncFunctionDef, ast.ClassDef)):
                for node in ast.walk(scope):
                    if isinstance(node, ast.ImportFrom) and node.level > 0:
                        found.add((os.path.basename(path), scope.name, node.lineno))
    # a nested scope reports its imports under every enclosing name: the allow-list names the outermost
    hidden = sorted(f for f in found if (f[0], f[1]) not in LOCAL_IMPORTS_ALLOWED)
    assert not hidden, hidden
    assert {(f[0], f[1]) for f in found} == LOCAL_IMPORTS_ALLOWED          # and no stale entry in the list


# ------------------------------------------------------------------------------------------------ registration
def _registry_of(key):
    """The registry (by its name) that the typed config under ``key`` is built from; None: not built through a registry."""
    if key in ('norm_cfg', 'nms', 'assigner', 'sampler'):
        return None             # BN / GN and nms are plain names; assigner and sampler belong to train_cfg (assigners.py)
    if key in ('roi_layer', 'shared_head', 'bbox_coder', 'neck', 'backbone'):
        return key
    if key == 'anchor_generator':
        return 'anchor generator'
    if key == 'upsample_cfg':
        return 'upsample'
    if key.endswith('roi_extractor'):
        return 'roi_extractor'
    if key.startswith('loss'):
        return 'loss'
    if key.endswith('head'):
        return 'head'
    raise AssertionError(f'a typed config under {key!r}: say in _registry_of which registry builds it')


def _typed(cfg, key, out):
    if isinstance(cfg, dict):
        if 'type' in cfg and _registry_of(key) is not None:
            out.add((_registry_of(key), cfg['type']))
        for k, v in cfg.items():
            _typed(v, k, out)
    elif isinstance(cfg, (list, tuple)):
        for v in cfg:
            _typed(v, key, out)
    return out


def _config_sections(golden_dir):
    """model part -> the sections of every tests/golden/*_configs.json."""
    parts = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, '*_configs.json'))):
        with open(path) as f:
            for cfg in json.load(f).values():
                for part, sec in cfg['model'].items():
                    parts.setdefault(part, []).append(sec)
    return parts


# PointRefineMaskHead keeps its loss config and builds none: the reference registers this loss nowhere (Quirk Q15)
NEVER_REGISTERED = {('loss', 'PointRefineCrossEntropyLoss')}


def test_importing_roi_head_alone_registers_what_its_configs_name(fresh, golden_dir):
    from dynamask_amd import synth
    wanted = set()
    for sec in _config_sections(golden_dir)['roi_head']:
        _typed(sec, 'roi_head', wanted)
    for name, key in (('MASK_ROI_EXTRACTOR_CFG', 'mask_roi_extractor'), ('BBOX_ROI_EXTRACTOR_CFG', 'bbox_roi_extractor'),
                      ('MASK_HEAD_CFG', 'mask_head'), ('FCN_HEAD_CFG', 'mask_head'), ('BBOX_HEAD_CFG', 'bbox_head')):
        _typed(getattr(synth, name), key, wanted)
    # the names synth's configs are built under (they carry no ``type`` of their own)
    wanted |= {('head', n) for n in ('DynaMaskRoIHead', 'StandardRoIHead', 'DynaMaskHead', 'FCNMaskHead', 'Shared2FCBBoxHead')}
    wanted.add(('roi_extractor', 'SingleRoIExtractor'))
    assert {r for r, _ in wanted} >= {'head', 'roi_extractor', 'loss', 'bbox_coder', 'shared_head'}
    regs = fresh['roi_head']['registries']
    missing = sorted((r, t) for r, t in wanted - NEVER_REGISTERED if t not in regs.get(r, ()))
    assert not missing, missing
    assert all(t not in regs[r] for r, t in NEVER_REGISTERED)


@pytest.mark.parametrize('part,module', [('rpn_head', 'dense_heads'), ('neck', 'necks'), ('backbone', 'backbones')])
def test_the_other_sections_register_with_their_own_module(fresh, golden_dir, part, module):
    wanted = set()
    for sec in _config_sections(golden_dir)[part]:
        _typed(sec, part, wanted)
    wanted = {(r, t) for r, t in wanted if r != 'loss'}         # RPNHead stores its loss configs and builds none
    assert wanted
    regs = fresh[module]['registries']
    missing = sorted((r, t) for r, t in wanted if t not in regs.get(r, ()))
    assert not missing, missing


# ------------------------------------------------------------------------------------------------ init is unchanged
@pytest.fixture(scope='module')
def recorded():
    with open(module_digest.FIXTURE) as f:
        return json.load(f)


def test_every_buildable_section_is_recorded(recorded):
    assert sorted(recorded) == sorted(SECTIONS)


@pytest.mark.parametrize('name', sorted(SECTIONS))
def test_section_starts_from_the_recorded_weights(recorded, name):
    got = module_digest.digest(SECTIONS[name])
    want = recorded[name]
    assert [k for k, _ in got['keys']] == [k for k, _ in want['keys']]
    assert got['keys'] == want['keys']
    assert got['sha256'] == want['sha256']


# ------------------------------------------------------------------------------------------------ the linear holder
@pytest.mark.parametrize('cin,cout', [(12544, 1024), (7, 3)])
def test_linear_holder_draws_as_torch_does(cin, cout):
    from dynamask_amd.layers import _FC, _Linear
    torch.manual_seed(11)
    m = _Linear(cin, cout)
    torch.manual_seed(11)
    ref = nn.Linear(cin, cout)
    assert torch.equal(m.weight, ref.weight) and torch.equal(m.bias, ref.bias)
    torch.manual_seed(11)
    x = _FC(cin, cout)
    torch.manual_seed(11)
    w = nn.init.xavier_uniform_(torch.empty(cout, cin))
    assert torch.equal(x.weight, w) and torch.equal(x.bias, torch.zeros(cout))
    for holder in (m, x):
        assert list(holder.state_dict()) == ['weight', 'bias'] and tuple(holder.weight.shape) == (cout, cin)
        assert (holder.in_features, holder.out_features) == (cin, cout)
        assert isinstance(holder.weight, nn.Parameter) and isinstance(holder.bias, nn.Parameter)
