"""The guard net's coverage, counted from include/dynamask_hip.h without a device: every entry point that takes a stream
is reached by a pass of test_guard_surface_gpu.py (``EXPECTED_REACHED``) or has no call site in the package
(``NO_CALL_SITE``) -- a kernel added to the header and to no pass fails here --, and ``LaunchLog``'s reading of the
argument roles against a fake library."""
import ctypes
import glob
import os
import re
import types

import pytest

import guard_arena as ga
from dynamask_amd import hazard

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'dynamask_amd')


def _launching():
    return ga.launching(hazard.parse_header())


def _package_sources():
    return {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(PACKAGE, '*.py')))}


def test_every_launching_entry_point_is_in_exactly_one_table():
    surface = _launching()
    assert len(surface) >= 125
    reached = set().union(*ga.EXPECTED_REACHED.values())
    both = reached & set(ga.NO_CALL_SITE)
    assert not both, f'in EXPECTED_REACHED and in NO_CALL_SITE: {sorted(both)}'
    covered = reached | set(ga.NO_CALL_SITE)
    assert surface - covered == set(), f'launching entry points of the header that no guard pass reaches: {sorted(surface - covered)}'
    assert covered - surface == set(), f'names in the tables that the header does not declare as launching: {sorted(covered - surface)}'


def test_a_name_deleted_from_the_table_is_noticed(monkeypatch):
    name = 'dm_conv2d_fwd'
    assert any(name in s for s in ga.EXPECTED_REACHED.values())
    monkeypatch.setattr(ga, 'EXPECTED_REACHED', {k: set(v) - {name} for k, v in ga.EXPECTED_REACHED.items()})
    with pytest.raises(AssertionError, match=name):
        test_every_launching_entry_point_is_in_exactly_one_table()


def test_no_call_site_names_have_none():
    sources = _package_sources()
    assert 'ops.py' in sources
    for name, reason in ga.NO_CALL_SITE.items():
        assert reason.strip()
        named_in = [f for f, text in sources.items() if re.search(rf'\b{name}\b', text)]
        assert not named_in, f'{name} is named in {named_in}: it has a call site, a pass must reach it'
    # the two call sites that take the name from a variable choose among literals of ops.py
    # (dm_roi_align_*_fwd / _fwd_ws and the three dm_conv2d_wgrad*): a third would have to be read here as well
    assert sum(text.count('getattr(lib()') for text in sources.values()) == sources['ops.py'].count('getattr(lib(), name)') == 2


def test_unguarded_stores_name_launching_store_arguments():
    roles = hazard.parse_header()
    for (name, arg), why in ga.UNGUARDED_STORES.items():
        assert name in _launching() and roles[name][arg] in ('out', 'out[]') and why.strip(), (name, arg)


# ------------------------------------------------------------------------------------------------ LaunchLog on a fake library
ROLES = {'dm_fake_launch': ['in', 'out', 'in[]', 'out[]', 'scalar', 'out', 'stream'],
         'dm_fake_host': ['in', 'out', 'scalar']}


class _FakeLib:
    def __init__(self):
        self.calls = []

    def dm_fake_launch(self, *args):
        self.calls.append(('dm_fake_launch', args))
        return 0

    def dm_fake_host(self, *args):
        self.calls.append(('dm_fake_host', args))
        return 7


def _fake(spans, proxy=False):
    real = _FakeLib()
    module = types.SimpleNamespace(_LIB=real, _PROXY=_FakeLib() if proxy else None)
    arena = types.SimpleNamespace(spans=list(spans))
    return real, module, ga.LaunchLog(arena, roles=ROLES, module=module)


def _vp(v):
    return ctypes.c_void_p(v)


def _arr(*vs):
    return (ctypes.c_void_p * len(vs))(*vs)


def test_launch_log_reads_the_roles():
    real, module, log = _fake([(1000, 2000), (5000, 5000), (8000, 8100)])
    with log:
        assert module._LIB is not real
        # every store pointer inside a block: the first byte, the middle (a channel slice), the last byte; null ones skipped
        assert module._LIB.dm_fake_launch(_vp(50), _vp(1000), _arr(1500, 60), _arr(1999, 8050, 0), 3, None, None) == 0
        assert log.reached_guarded() == {'dm_fake_launch'} and log.unguarded_stores() == set()
        # one past the end of a block, in an out[] array; an empty block holds its own address
        module._LIB.dm_fake_launch(None, _vp(5000), None, _arr(1500, 2000), 3, _vp(0), None)
        assert log.unguarded_stores() == {('dm_fake_launch', 3)}
        # a scalar that looks like an address is no pointer; in front of the first block
        module._LIB.dm_fake_launch(_vp(1200), _vp(999), _arr(), _arr(), 1500, _vp(8099), None)
        assert log.unguarded_stores() == {('dm_fake_launch', 3), ('dm_fake_launch', 1)}
        # entry points without a stream are handed through unlogged
        assert module._LIB.dm_fake_host(_vp(1), _vp(2), 3) == 7
    assert module._LIB is real and module._PROXY is None
    assert log.launches == {'dm_fake_launch': 3} and log.guarded_launches == {'dm_fake_launch': 1}
    assert log.stores == {('dm_fake_launch', 1): [2, 1], ('dm_fake_launch', 3): [3, 1], ('dm_fake_launch', 5): [1, 0]}
    assert log.reads == {('dm_fake_launch', 0): [1, 1], ('dm_fake_launch', 2): [1, 1]}
    assert [n for n, _ in real.calls] == ['dm_fake_launch'] * 3 + ['dm_fake_host']
    n, stores, reads = log.shares()
    assert n == 3 and stores == 6 / 8 and reads == 2 / 4


def test_launch_log_sees_blocks_allocated_after_it_was_installed_and_wraps_the_hazard_proxy():
    real, module, log = _fake([], proxy=True)
    proxy = module._PROXY
    with log:
        assert module._PROXY is not proxy
        module._PROXY.dm_fake_launch(None, _vp(4096), None, None, 0, None, None)
        log.arena.spans.append((4096, 4100))
        module._PROXY.dm_fake_launch(None, _vp(4096), None, None, 0, None, None)
    assert module._LIB is real and module._PROXY is proxy
    assert log.stores == {('dm_fake_launch', 1): [1, 1]} and len(proxy.calls) == 2 and not real.calls


def test_launch_log_restores_the_library_when_the_block_raises():
    real, module, log = _fake([])
    with pytest.raises(ZeroDivisionError):
        with log:
            1 / 0
    assert module._LIB is real
