"""Every build and every route of the DCN forward launcher (csrc/deform_conv.hip: dcn_route / dcn_emit) against the oracle.

Each case names a route -- one of the 13 gather instantiations launched alone, or "LDS + split", "band + split", "c256 + seam",
"LDS + seam" -- and a map; the batch is the smallest whose plan (ops.deform_conv_plan: the launcher's own route on this
device's compute-unit count, nothing restated here) names that route.  Every variant forms the same products in the same
order, so on the routes that do not split the K loop EVERY row is compared bit for bit with 3-RoI launches of the same rows;
on all routes the first and the last RoI go against ref_ops.deform_conv2d through the project's fp64 triangle
(tolerances.assert_close_via_f64).  Offsets as in tests/test_dcn_c256_gpu.py: void taps, border clamps and a far row.
16 input channels (two K chunks, two deformable groups); the split routes need 64: dcn_choose_split's cost model asks for
more than 26 us of K loop (8 chunks) before a split pays."""
import functools

import pytest
import torch

from oracle import ref_ops
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

GENERIC, LDS, C256, BAND = range(4)
BUILDS = [(GENERIC, 1, 4, 1, 1), (GENERIC, 2, 2, 1, 1), (GENERIC, 2, 2, 2, 1), (LDS, 0, 0, 0, 0), (C256, 0, 0, 0, 0),
          (BAND, 1, 2, 4, 0), (BAND, 1, 2, 7, 0), (BAND, 2, 1, 4, 0), (BAND, 2, 1, 7, 0),
          (BAND, 1, 4, 4, 0), (BAND, 1, 4, 7, 0), (BAND, 4, 1, 4, 0), (BAND, 2, 2, 7, 0)]
# (id, build of the first launch, 'plain' / 'split' / 'seam', H, W, Cout, C): the map and channel counts on which the route exists
CASES = [('32x128', BUILDS[0], 'plain', 7, 7, 20, 16),
         ('64x64', BUILDS[1], 'plain', 7, 7, 40, 16),
         ('128x64', BUILDS[2], 'plain', 7, 7, 72, 16),
         ('lds', BUILDS[3], 'plain', 14, 14, 72, 16),
         ('c256', BUILDS[4], 'plain', 14, 14, 232, 16),
         ('band<1,2,4>', BUILDS[5], 'plain', 16, 28, 40, 16),
         ('band<1,2,7>', BUILDS[6], 'plain', 16, 36, 40, 16),
         ('band<2,1,4>', BUILDS[7], 'plain', 16, 28, 40, 16),
         ('band<2,1,7>', BUILDS[8], 'plain', 16, 36, 40, 16),
         ('band<1,4,4>', BUILDS[9], 'plain', 16, 28, 100, 16),
         ('band<1,4,7>', BUILDS[10], 'plain', 16, 36, 100, 16),
         ('band<4,1,4>', BUILDS[11], 'plain', 16, 28, 100, 16),
         ('band<2,2,7>', BUILDS[12], 'plain', 16, 36, 100, 16),
         ('lds+split', BUILDS[3], 'split', 14, 14, 72, 64),
         ('band+split', BUILDS[7], 'split', 16, 28, 40, 64),
         ('c256+seam', BUILDS[4], 'seam', 14, 14, 232, 16),
         ('lds+seam', BUILDS[3], 'seam', 14, 14, 72, 16)]
DG = 2
MIN_NB, MAX_NB = 5, 1500


@pytest.fixture(scope='module')
def ops():
    from dynamask_amd import ops as o
    assert o.CONV_SPLITK[0], 'DM_CONV_SPLITK=0: the split routes cannot be reached through ops.deform_conv'
    return o


def _build(rec):
    return (rec['kernel'], rec['P0'], rec['P1'], rec['P2'], rec['P3'])


def _plan(nb, C, H, W, cout, split):
    """The plan of the call ops.deform_conv makes: inside ops.splitk_scope with the workspace it allocates there."""
    from dynamask_amd import _lib, ops as o
    ws = int(_lib.lib().dm_deform_conv_splitk_floats(nb, C, H, W, cout)) if split else 0
    return o.deform_conv_plan(nb, C, H, W, cout, DG, workspace_floats=ws)


@functools.lru_cache(maxsize=None)
def _find(case):
    """(smallest batch whose plan is the case's route, that plan) -- from MIN_NB RoIs on: more than one 3-RoI launch to
    compare with, more than one workgroup, tiles that span two images"""
    _, build, kind, H, W, cout, C = case
    for nb in range(MIN_NB, MAX_NB):
        recs = _plan(nb, C, H, W, cout, kind == 'split')
        if _build(recs[0]) != build or len(recs) != (2 if kind == 'seam' else 1):
            continue
        if (recs[0]['ksplit'] > 1) == (kind == 'split'):
            return nb, recs
    raise AssertionError(f'no batch below {MAX_NB} takes the route {case[0]} on this device')


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(N, C, H, W, cout, seed):
    x = torch.randn(N, C, H, W, generator=_g(700 + seed))
    off = torch.randn(N, 18 * DG, H, W, generator=_g(701 + seed)) * 1.5
    off[0, :, 0, 0] = 40.0                       # far outside: all taps void
    off[-1, ::2, H // 2] = 25.0                  # a row of pixels looks 25 rows down / up: clamps at the borders
    off[-1, ::2, H // 2 + 1] = -25.0
    off[-1, :, -1, -1] = -3.25
    w = torch.randn(cout, C, 3, 3, generator=_g(702 + seed)) / (9 * C) ** 0.5
    return x, off, w


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_route_matches_small_launches_and_the_oracle(ops, case):
    name, build, kind, H, W, cout, C = case
    N, recs = _find(case)
    if kind == 'seam':
        main, tail = recs
        assert _build(tail) == BUILDS[1] and main['q_begin'] == 0 and main['Q'] == tail['q_begin'] and tail['Q'] == N * H * W
    if kind == 'split':
        assert recs[0]['reduce'] == 1 and recs[0]['grid_y'] == recs[0]['ksplit'] >= 2
    x, off, w = _inputs(N, C, H, W, cout, CASES.index(case))
    xd, offd = x.cuda(), off.cuda()
    wq = ops.pack_conv_weight(w.cuda())
    if kind == 'split':
        with ops.splitk_scope():
            out = ops.deform_conv(xd, offd, wq, cout, DG)
    else:
        out = ops.deform_conv(xd, offd, wq, cout, DG)
        # (3 RoIs: a launch of its own route -- the plan says which; never this one's seam or split)
        small = torch.cat([ops.deform_conv(xd[s:s + 3].contiguous(), offd[s:s + 3].contiguous(), wq, cout, DG) for s in range(0, N, 3)])
        assert torch.equal(out, small), name
    sel = [0, N - 1]
    r32 = ref_ops.deform_conv2d(x[sel], off[sel], w, 1, 1, 1, DG)
    r64 = ref_ops.deform_conv2d(x[sel].double(), off[sel].double(), w.double(), 1, 1, 1, DG)
    assert_close_via_f64(out[sel].cpu(), r32, r64, name=f'dcn {name} {H}x{W} cout={cout} N={N}')


def test_the_cases_cover_every_build_and_route(ops):
    found = {c[0]: _find(c)[1] for c in CASES}
    assert {_build(r) for recs in found.values() for r in recs} == set(BUILDS)
    assert {c[1] for c in CASES if c[2] == 'plain'} == set(BUILDS) and len(BUILDS) == 13
    assert {(c[1][0], c[2]) for c in CASES if c[2] != 'plain'} == {(LDS, 'split'), (BAND, 'split'), (C256, 'seam'), (LDS, 'seam')}
