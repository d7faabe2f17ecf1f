"""CARAFE on the MI355X, every way dm_carafe_fwd / dm_carafe_bwd can run (csrc/carafe.hip): the LDS tile kernel at
channel-tile widths 32, 16 and 4, its fallback to the generic kernel when the tile exceeds LDS, the generic kernel by
each of its three entry conditions (H*W > 256, cpg % 4 != 0, scale != 2), up_kernel 3 and 5, group 1 and 2, and the
three backward kernels at ragged shapes.  The reference is oracle.ref_ops.carafe_reassemble on
softmax(pixel_shuffle(enc)) in float32 and float64 on the CPU (autograd of the float64 form for the gradients),
compared through the triangle of tests/tolerances.py.  Every case works its path out from the dispatch rule restated
here and asserts it, so that a later change to the rule cannot silently move a case.  Every output (and the backward's
scratch) is written between two canary guard bands that must survive."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops
from tolerances import assert_close_via_f64

pytestmark = pytest.mark.gpu

CANARY = 7.0
GUARD = 4096
OK, INVALID_ARG, UNSUPPORTED = 0, -1, -3        # DM_OK, DM_ERR_INVALID_ARG, DM_ERR_UNSUPPORTED of include/dynamask_hip.h
LDS_LIMIT = 64 * 1024


class Guarded:
    """A device tensor of ``shape`` between two guard bands of CANARY (the tensor itself starts as CANARY too)."""

    def __init__(self, shape, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), CANARY, device='cuda')
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        if fill is not None:
            self.t.copy_(fill)

    def check(self, what):
        torch.cuda.synchronize()
        n = self.t.numel()
        assert bool((self.buf[:GUARD] == CANARY).all()), f'{what}: the guard band before the output was overwritten'
        assert bool((self.buf[GUARD + n:] == CANARY).all()), f'{what}: the guard band past the output was overwritten'

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == CANARY).all())


def _lib():
    from dynamask_amd._lib import lib
    return lib()


def _call_fwd(x, enc, k, group, scale, out, NB=None):
    from dynamask_amd import ops
    nb, C, H, W = x.shape
    return _lib().dm_carafe_fwd(ops._p(x), ops._p(enc), nb if NB is None else NB, C, H, W, k, group, scale, ops._p(out),
                                ops._stream())


def _call_bwd(x, enc, go, k, group, scale, gx, genc, scratch):
    from dynamask_amd import ops
    NB, C, H, W = x.shape
    return _lib().dm_carafe_bwd(ops._p(x), ops._p(enc), ops._p(go), NB, C, H, W, k, group, scale, ops._p(gx), ops._p(genc),
                                ops._p(scratch), ops._stream())


# ------------------------------------------------------------------------------------------------ the dispatch rule
def _channel_tile(cpg):
    return 32 if cpg % 32 == 0 else 16 if cpg % 16 == 0 else 4 if cpg % 4 == 0 else 0


def _tile_bytes(ct, H, W, k):
    return (ct // 4) * (H + 2 * (k // 2)) * (W + 2 * (k // 2)) * 16          # float4 slots of the zero-padded tile


def fwd_path(C, H, W, k, group, scale):
    """dm_carafe_fwd's rule restated: ('tile', CTt) | ('fallback', CTt) | ('generic', reasons)."""
    cpg = C // group
    ct = _channel_tile(cpg)
    reasons = tuple(r for r, hit in (('hw', H * W > 256), ('cpg', ct == 0), ('scale', scale != 2)) if hit)
    if reasons:
        return 'generic', reasons
    return ('tile' if _tile_bytes(ct, H, W, k) <= LDS_LIMIT else 'fallback'), ct


# (NB, C, H, W, k, group, scale) -> the path the case must take
FWD_CASES = [
    ((2, 64, 14, 14, 3, 2, 2), ('tile', 32)),            # k = 3, two groups
    ((2, 48, 11, 12, 5, 1, 2), ('tile', 16)),            # three chunks, H*W = 132: no multiple of 64
    ((2, 24, 16, 16, 5, 2, 2), ('tile', 4)),             # H*W = 256: every thread active
    ((1, 8, 1, 200, 5, 1, 2), ('tile', 4)),              # one-row map
    ((2, 8, 5, 7, 3, 2, 2), ('tile', 4)),                # odd W: the float2 stores stay 8-byte aligned (the row pitch is 2W)
    ((1, 32, 1, 256, 5, 1, 2), ('fallback', 32)),        # 8 x 5 x 260 float4 > 64 KB
    ((2, 20, 17, 16, 5, 1, 2), ('generic', ('hw',))),    # H*W = 272; channel chunks 16 + 4; ragged last pixel block
    ((2, 6, 5, 7, 3, 2, 2), ('generic', ('cpg',))),      # cpg = 3, k = 3, two groups
    ((2, 8, 3, 4, 5, 2, 3), ('generic', ('scale',))),    # scale 3
]
BWD_CASES = [(2, 64, 14, 14, 3, 2), (2, 48, 11, 12, 5, 1), (2, 24, 16, 16, 5, 2), (1, 8, 1, 200, 5, 1), (3, 256, 14, 14, 5, 1),
             (2, 8, 5, 7, 3, 2), (1, 4, 3, 5, 5, 1)]        # odd W (the float2 loads of grad_out: row pitch 2W, always even)


def _id(case):
    return 'x'.join(str(v) for v in case)


def test_cases_cover_every_path():
    """Between them the forward cases reach the tile kernel at 32, 16 and 4, the LDS fallback, the generic kernel by each
    entry condition alone, k = 3 and k = 5 on both kernels, and group 1 and 2 on both kernels."""
    seen = set()
    for (NB, C, H, W, k, group, scale), path in FWD_CASES:
        assert fwd_path(C, H, W, k, group, scale) == path
        kernel = 'tile' if path[0] == 'tile' else 'generic'
        seen |= {path, (kernel, 'k', k), (kernel, 'group', group)}
    want = {('tile', 32), ('tile', 16), ('tile', 4), ('fallback', 32), ('generic', ('hw',)), ('generic', ('cpg',)),
            ('generic', ('scale',))}
    want |= {(kern, 'k', k) for kern in ('tile', 'generic') for k in (3, 5)}
    want |= {(kern, 'group', g) for kern in ('tile', 'generic') for g in (1, 2)}
    assert want <= seen, want - seen


# ------------------------------------------------------------------------------------------------ references (once)
def _reassemble(x, enc, k, group, scale):
    NB, _, H, W = x.shape
    m = F.pixel_shuffle(enc, scale)
    m = F.softmax(m.view(NB, group, k * k, H * scale, W * scale), dim=2).view(NB, group * k * k, H * scale, W * scale)
    return ref_ops.carafe_reassemble(x, m, k, group, scale)


@functools.lru_cache(maxsize=None)
def _inputs(NB, C, H, W, k, group, scale):
    g = torch.Generator().manual_seed(1000 + NB + 3 * C + 5 * H + 7 * W + 11 * k + 13 * group + 17 * scale)
    x = torch.randn(NB, C, H, W, generator=g)
    enc = torch.randn(NB, k * k * group * scale * scale, H, W, generator=g) * 1.5      # a softmax that is far from uniform
    go = torch.randn(NB, C, H * scale, W * scale, generator=g)
    return x, enc, go


@functools.lru_cache(maxsize=None)
def _fwd_ref(*case):
    x, enc, _ = _inputs(*case)
    k, group, scale = case[4:]
    with torch.no_grad():
        return _reassemble(x, enc, k, group, scale), _reassemble(x.double(), enc.double(), k, group, scale)


@functools.lru_cache(maxsize=None)
def _bwd_ref(*case):
    """(grad_x, grad_enc) by autograd of the float32 and of the float64 form."""
    x, enc, go = _inputs(*case)
    k, group, scale = case[4:]
    res = []
    for dt in (torch.float32, torch.float64):
        xr, er = x.detach().clone().to(dt).requires_grad_(True), enc.detach().clone().to(dt).requires_grad_(True)
        _reassemble(xr, er, k, group, scale).backward(go.to(dt))
        res.append((xr.grad, er.grad))
    return res


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize('case,path', FWD_CASES, ids=[_id(c) for c, _ in FWD_CASES])
def test_carafe_forward(case, path):
    NB, C, H, W, k, group, scale = case
    assert fwd_path(C, H, W, k, group, scale) == path
    x, enc, _ = _inputs(*case)
    xd, ed = x.cuda(), enc.cuda()
    out = Guarded((NB, C, H * scale, W * scale))
    assert _call_fwd(xd, ed, k, group, scale, out.t) == OK
    out.check(f'carafe {_id(case)}')
    assert torch.equal(xd.cpu(), x) and torch.equal(ed.cpu(), enc), 'an input was modified'
    r32, r64 = _fwd_ref(*case)
    err, ref_err, scale_ = assert_close_via_f64(out.t, r32, r64, f'carafe {_id(case)} {path}')
    print(f'carafe fwd {_id(case)} {path}: |product - f64| {err:.3g}, fp32 reference {ref_err:.3g}, scale {scale_:.3g}')
    again = Guarded(out.t.shape)
    assert _call_fwd(xd, ed, k, group, scale, again.t) == OK
    again.check('second run')
    assert torch.equal(out.t, again.t), 'two runs differ'
    # nothing splits a sum across samples: each sample's rows are those of a one-sample launch, bit for bit
    for n in range(NB):
        one = Guarded((1, C, H * scale, W * scale))
        assert _call_fwd(xd[n:n + 1].contiguous(), ed[n:n + 1].contiguous(), k, group, scale, one.t) == OK
        one.check(f'sample {n} alone')
        assert torch.equal(one.t[0], out.t[n]), f'sample {n} of the batch differs from its one-sample launch'


@pytest.mark.parametrize('case,path', FWD_CASES, ids=[_id(c) for c, _ in FWD_CASES])
def test_carafe_constant_enc_is_the_zero_padded_box_mean(case, path):
    """A constant enc gives the uniform kernel 1 / k^2: the output is the box sum of the zero-padded x over k x k, over
    k^2, at every sub-pixel -- border pixels lose the mass that falls outside the image and are not renormalised."""
    NB, C, H, W, k, group, scale = case
    x, _, _ = _inputs(*case)
    enc = torch.full((NB, k * k * group * scale * scale, H, W), 0.37)
    out = Guarded((NB, C, H * scale, W * scale))
    assert _call_fwd(x.cuda(), enc.cuda(), k, group, scale, out.t) == OK
    out.check('constant enc')

    def box(t):
        s = F.avg_pool2d(t, k, stride=1, padding=k // 2, count_include_pad=True)          # sum over k x k of padded x / k^2
        return s.repeat_interleave(scale, dim=2).repeat_interleave(scale, dim=3)
    assert_close_via_f64(out.t, box(x), box(x.double()), f'box mean {_id(case)}')
    # a corner pixel sees (k//2 + 1)^2 of the k^2 taps (fewer on maps narrower than the kernel): its mass is NOT spread
    # over the taps that remain
    ones = Guarded((NB, C, H * scale, W * scale))
    assert _call_fwd(torch.ones_like(x).cuda(), enc.cuda(), k, group, scale, ones.t) == OK
    assert_close_via_f64(ones.t, box(torch.ones_like(x)), box(torch.ones_like(x).double()), f'box mean of ones {_id(case)}')
    r = k // 2
    inside = (min(r, H - 1) + 1) * (min(r, W - 1) + 1)
    assert inside < k * k
    corner = ones.t[:, :, 0, 0].cpu()
    assert float(corner.max()) < 1.0 - 0.5 / (k * k) and float(corner.min()) > (inside - 0.5) / (k * k), \
        f'corner {float(corner[0, 0]):.6g}, {inside} of {k * k} taps inside: the border was renormalised'


def test_carafe_forward_edges_and_refusals():
    x = torch.randn(2, 8, 5, 6, device='cuda')
    enc = torch.randn(2, 100, 5, 6, device='cuda')
    out = Guarded((2, 8, 10, 12))
    assert _call_fwd(x, enc, 5, 1, 2, out.t, NB=0) == OK
    assert out.untouched(), 'NB = 0 wrote something'
    enc7 = torch.randn(2, 49 * 4, 5, 6, device='cuda')
    assert _call_fwd(x, enc7, 7, 1, 2, out.t) == UNSUPPORTED
    assert out.untouched(), 'up_kernel = 7 wrote something'
    enc3 = torch.randn(2, 100 * 3, 5, 6, device='cuda')
    assert _call_fwd(x, enc3, 5, 3, 2, out.t) == INVALID_ARG                 # C % group != 0
    assert out.untouched(), 'C % group != 0 wrote something'


def test_ops_carafe_wrappers_reach_the_generic_kernel():
    """ops.carafe / ops.carafe_backward (the callers' entry points) on a generic-path shape and on a refused backward."""
    from dynamask_amd import ops
    case = (2, 20, 17, 16, 5, 1, 2)
    x, enc, go = _inputs(*case)
    r32, r64 = _fwd_ref(*case)
    assert_close_via_f64(ops.carafe(x.cuda(), enc.cuda(), 5, 1, 2), r32, r64, 'ops.carafe generic')
    with pytest.raises(RuntimeError, match='dm_carafe_bwd'):
        ops.carafe_backward(x.cuda(), enc.cuda(), go.cuda(), 5, 1, 2)


# ------------------------------------------------------------------------------------------------ backward
def _scratch_floats(NB, H, W, k, group):
    return int(_lib().dm_carafe_bwd_scratch_floats(NB, H, W, k, group))


def _run_bwd(case, xd, ed, gd):
    NB, C, H, W, k, group = case
    gx, genc = Guarded(xd.shape), Guarded(ed.shape)
    n_scr = _scratch_floats(NB, H, W, k, group)
    assert n_scr == NB * group * 4 * k * k * H * W
    scratch = Guarded((n_scr,))
    assert _call_bwd(xd, ed, gd, k, group, 2, gx.t, genc.t, scratch.t) == OK
    for gb, name in ((gx, 'grad_x'), (genc, 'grad_enc'), (scratch, 'scratch')):
        gb.check(f'carafe backward {_id(case)} {name}')
    return gx, genc


@pytest.mark.parametrize('case', BWD_CASES, ids=[_id(c) for c in BWD_CASES])
def test_carafe_backward(case):
    NB, C, H, W, k, group = case
    cpg = C // group
    ct = _channel_tile(cpg)
    # the backward's support rule: scale 2, H*W <= 256, cpg % 4 == 0, and the x tile of CT channels within LDS
    assert H * W <= 256 and ct > 0 and _tile_bytes(ct, H, W, k) <= LDS_LIMIT
    x, enc, go = _inputs(*case, 2)
    xd, ed, gd = x.cuda(), enc.cuda(), go.cuda()
    gx, genc = _run_bwd(case, xd, ed, gd)
    assert torch.equal(xd.cpu(), x) and torch.equal(ed.cpu(), enc) and torch.equal(gd.cpu(), go), 'an input was modified'
    (gx32, ge32), (gx64, ge64) = _bwd_ref(*case, 2)
    for got, r32, r64, name in ((gx.t, gx32, gx64, 'grad_x'), (genc.t, ge32, ge64, 'grad_enc')):
        err, ref_err, scale_ = assert_close_via_f64(got, r32, r64, f'carafe backward {_id(case)} {name}')
        allowed = max(ref_err, 1e-4 * min(scale_, 1.0))
        print(f'carafe bwd {_id(case)} {name}: |product - f64| {err:.3g}, allowed {allowed:.3g} + 1e-4 |f64| '
              f'(fp32 reference {ref_err:.3g}, scale {scale_:.3g})')
    gx2, genc2 = _run_bwd(case, xd, ed, gd)
    assert torch.equal(gx.t, gx2.t), 'grad_x is a gather: two runs must give the same bits'
    if cpg == ct:
        # one chunk covers the group: every scratch cell receives one atomic add onto zero
        assert torch.equal(genc.t, genc2.t), 'grad_enc: one chunk per group, two runs must give the same bits'
    else:
        assert_close_via_f64(genc2.t, ge32, ge64, f'carafe backward {_id(case)} grad_enc, second run')


def test_backward_cases_cover_one_and_several_chunks():
    chunks = {(C // group) // _channel_tile(C // group) for _, C, _, _, _, group in BWD_CASES}
    assert 1 in chunks and max(chunks) > 1
    assert (2, 64, 14, 14, 3, 2) in BWD_CASES and 64 // 2 == _channel_tile(64 // 2)


# (NB, C, H, W, k, group, scale): why dm_carafe_bwd refuses it
BWD_REFUSED = [((2, 8, 3, 4, 5, 2, 3), 'scale 3'), ((2, 20, 17, 16, 5, 1, 2), 'H*W = 272'), ((2, 6, 5, 7, 3, 2, 2), 'cpg = 3'),
               ((2, 8, 5, 6, 7, 1, 2), 'k = 7'), ((1, 32, 1, 256, 5, 1, 2), 'the 32-channel tile exceeds LDS')]


@pytest.mark.parametrize('case,why', BWD_REFUSED, ids=[w for _, w in BWD_REFUSED])
def test_carafe_backward_refusals(case, why):
    NB, C, H, W, k, group, scale = case
    if why.startswith('the 32-channel'):
        assert _channel_tile(C // group) == 32 and _tile_bytes(32, H, W, k) > LDS_LIMIT and H * W <= 256
    g = torch.Generator().manual_seed(5)
    x = torch.randn(NB, C, H, W, generator=g).cuda()
    enc = torch.randn(NB, k * k * group * scale * scale, H, W, generator=g).cuda()
    go = torch.randn(NB, C, H * scale, W * scale, generator=g).cuda()
    gx, genc = Guarded(x.shape), Guarded(enc.shape)
    scratch = Guarded((max(_scratch_floats(NB, H, W, k, group), 1),))
    assert _call_bwd(x, enc, go, k, group, scale, gx.t, genc.t, scratch.t) == UNSUPPORTED, why
    assert gx.untouched() and genc.untouched(), f'{why}: a refused call wrote to its outputs'
    assert scratch.untouched(), f'{why}: a refused call wrote to its scratch'


def test_carafe_backward_nb0_and_bad_group():
    x = torch.randn(2, 8, 5, 6, device='cuda')
    enc = torch.randn(2, 100, 5, 6, device='cuda')
    go = torch.randn(2, 8, 10, 12, device='cuda')
    from dynamask_amd import ops
    gx, genc, scratch = Guarded(x.shape), Guarded(enc.shape), Guarded((2 * 100 * 30,))
    L = _lib()
    args = lambda NB, group: (ops._p(x), ops._p(enc), ops._p(go), NB, 8, 5, 6, 5, group, 2, ops._p(gx.t), ops._p(genc.t),      # noqa: E731
                              ops._p(scratch.t), ops._stream())
    assert L.dm_carafe_bwd(*args(0, 1)) == OK
    assert L.dm_carafe_bwd(*args(2, 3)) == INVALID_ARG
    assert gx.untouched() and genc.untouched() and scratch.untouched()
